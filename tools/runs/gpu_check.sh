set -o pipefail
# D: output directory (outside the tree by default)
D=${D:-${TMPDIR:-/tmp}/netrep_gpu_check}; mkdir -p $D
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $D/pytest_gpu.txt 2>&1 && \
timeout -k 10 300 python -u bench.py --full > $D/bench.json 2> $D/bench.err
