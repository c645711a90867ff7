# usage: bash tools/ab_variants.sh name1 name2 ...   (libraries zkp-ecdsa_amd/build_ab/lib_<name>.so; "base" here = lib_base.so, "main" = the built library)
# AB_ARGS: extra bench.py arguments (default: no host-buffer pass)
O=${OUT_DIR:-out}   # output folder, relative to the repository root
mkdir -p $O/ab
for v in "$@"; do
  lib=$PWD/zkp-ecdsa_amd/build_ab/lib_$v.so
  [ "$v" = main ] && lib=$PWD/zkp-ecdsa_amd/lib/libzkattest_hip.so
  ZKATTEST_LIB=$lib timeout 300 python bench.py --full --no-cpu-baseline --steps 2 --warmup 1 ${AB_ARGS:---host-io 0} > $O/ab/$v.json 2> $O/ab/$v.err
  echo "$v rc=$?"
done
