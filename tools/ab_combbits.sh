O=${OUT_DIR:-out}   # output folder, relative to the repository root
mkdir -p $O/abw
for v in 24 22 20 18 24; do
  timeout 300 python bench.py --full --no-cpu-baseline --verify-steps 0 --steps 1 --warmup 1 --comb-bits $v > $O/abw/w$v.json 2> $O/abw/w$v.err
  echo "$v rc=$?"
done
