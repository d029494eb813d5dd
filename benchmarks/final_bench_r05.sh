OUT=${1:-bench_out/r05}
mkdir -p $OUT
python bench.py --full > $OUT/bench_n1.json 2> $OUT/bench_n1.err; echo "n1 rc=$?"
python -c "from tests import mock_rccl; mock_rccl.build()"
FZ_RCCL_LIB=$PWD/tests/libmock_rccl.so FZ_DEVICES=0,0,0,0,0,0,0,0 python bench.py --gpus 8 --mib 1024 --no-cpu-baseline > $OUT/bench_8_ranks_stand_in.json 2> $OUT/bench_8.err; echo "8 ranks rc=$?"
FZ_DEVICES=0,0 python bench.py --gpus 2 --no-cpu-baseline > $OUT/bench_two_device_states.json 2> $OUT/bench_2.err; echo "2 states rc=$?"
python benchmarks/api_overhead.py > $OUT/api_overhead.txt 2>&1; echo "api rc=$?"
python bench.py --two-streams --no-cpu-baseline --no-extras > $OUT/bench_two_streams.json 2>/dev/null; echo "2 streams rc=$?"
