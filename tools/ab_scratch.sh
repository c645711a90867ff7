O=${OUT_DIR:-out}   # output folder, relative to the repository root
mkdir -p $O/abs
python bench.py --full --no-cpu-baseline --host-io 0 --steps 1 > $O/abs/d1.json 2>/dev/null
HSA_SCRATCH_SINGLE_LIMIT=4000000000 python bench.py --full --no-cpu-baseline --host-io 0 --steps 1 > $O/abs/lim.json 2>/dev/null
python bench.py --full --no-cpu-baseline --host-io 0 --steps 1 > $O/abs/d2.json 2>/dev/null
python bench.py --full --no-cpu-baseline --host-io 0 --steps 1 --lanes 1 > $O/abs/l1.json 2>/dev/null
rocm-smi --showmeminfo vram 2>/dev/null | head -5
