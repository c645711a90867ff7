O=${OUT_DIR:-out}   # output folder, relative to the repository root
mkdir -p $O/hio
for cfg in "16384 32768" "16384 4096" "16384 2048" "65536 8192"; do set -- $cfg
 python bench.py --full --no-cpu-baseline --verify-steps 0 --steps 1 --host-io $1 --host-io-chunk $2 > $O/hio/h_$1_$2.json 2> $O/hio/h_$1_$2.err; echo "$cfg rc=$?"
done
