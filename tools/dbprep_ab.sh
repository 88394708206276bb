# A/B of the two dbprep kernels on an MI355X, from the repository root: the hooks build with H264MI_DBPREP_GENERIC=1 (every launch on k_dbprep, as before
# there was k_dbprep_ip) and without (I / P launches on k_dbprep_ip).  Per variant one rocprofv3 kernel trace of the serialized bench; prints the dbprep and
# entropy rows of its kernel statistics (name, calls, total ns, average ns).
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd /tmp && export TMPDIR=/tmp
for v in 1 0; do
  out=$(mktemp -d /tmp/dbprep_ab_XXXXXX)
  H264MI_DBPREP_GENERIC=$v H264MI_LIB=$R/h264decode_amd/libh264mi_hooks.so timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out -o t -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-extra --no-cpu-baseline --no-parity --distinct 32 --serialized > $out/bench.json 2> $out/err.txt || { tail -3 $out/err.txt; exit 1; }
  f=$(find $out -name "*kernel_stats.csv" | head -1)
  echo "H264MI_DBPREP_GENERIC=$v"; grep "k_dbprep\|k_entropy" $f | cut -d, -f1-4
  rm -rf $out
done
