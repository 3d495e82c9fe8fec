"""ASan + UBSan over the host C / C++ (SURVEY §5 "Race detection / sanitizers"): `make -C oracle
sanitize` builds the oracle, the ABI's host half (csrc/dpg_host.c), the workload generator
(csrc/dpg_synth.c), the symbolic Cholesky (csrc/dpg_chol_sym.cpp) and the GPU solver's host planner
with the pick of the partial refactorization (csrc/dpg_chol_plan.cpp) and change detection's host
plan (csrc/dpg_change_plan.cpp: window reuse, bit-plane slots, candidates, against hand-worked values) with
-fsanitize=address,undefined -fno-sanitize-recover=all and runs tools/sanitize_check.cpp through them (scans -> clouds -> ICP -> GN -> symbolic analysis, full and
incremental -> solver plans of a mesh with team fronts and of a loop graph, every option set ->
the pick of both graphs before and after a node is appended, its runs applied on the host ->
DPG change detection), after the growth rules and ownership of the GPU layer's buffer template
(csrc/dpg_buf.h) over a counting malloc policy; any report fails the run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_under_asan_ubsan():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "sanitize"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "sanitize check ok" in r.stdout and "solver plans ok" in r.stdout and "partial pick ok" in r.stdout and "buffers ok" in r.stdout and "lists ok" in r.stdout and "change plan ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
