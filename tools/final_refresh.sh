set -x
out=$(realpath -m -- "${1:?usage: tools/final_refresh.sh <output directory>}"); mkdir -p "$out"     # (absolute: the next line changes directory)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout 1200 python -m pytest tests -m gpu -q 2>&1 | tail -3 > $out/tests.txt
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $out/smoke.txt 2>&1
timeout 400 python bench.py --full > $out/bench.json 2> $out/bench.err
timeout 300 python bench.py --full --no-cpu-baseline --host-inputs 2>/dev/null | tail -1 > $out/host_inputs.txt
timeout 300 python bench.py --mode inference --steps 10 --warmup 2 2>/dev/null | tail -1 > $out/inference.json
timeout 600 rocprofv3 --kernel-trace --stats -d $out/prof -o r01j -- python bench.py --full --no-cpu-baseline > $out/prof.log 2>&1
python tools/rocprof_summary.py $(ls $out/prof/*/*results.db $out/prof/*results.db 2>/dev/null | head -1) > $out/kernel_stats.txt 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 600 rocprofv3 --pmc $c -d $out/pmc_$c -o pmc --output-format csv -- python bench.py --full --no-cpu-baseline --no-graph --steps 2 --warmup 1 > $out/pmc_$c.log 2>&1
  python tools/pmc_family.py $out/pmc_$c conv_igemm wgrad_dma > $out/pmc_$c.txt 2>&1
done
rm -rf $out/prof $out/pmc_FETCH_SIZE $out/pmc_WRITE_SIZE
cat $out/tests.txt $out/smoke.txt; cut -c1-220 $out/bench.json; cat $out/pmc_*.txt; head -5 $out/kernel_stats.txt
