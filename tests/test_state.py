"""The record of what a model's derived buffers hold (csrc/mfgp_state.h), on the host:
tests/state_main.cpp includes that header alone, is compiled here with the host compiler
under AddressSanitizer and UBSan and run as a program of its own. It drives every event
and reads every predicate after it; checks that a truncate followed by an append back to
the same row count finds no posterior and no column-store row beyond the cut, the three
differences between rows_cut and restore_from with both outcomes of each, that a drop
inside a planner's loop trips restore_from's invariant, that a new generation empties the
generation-tagged buffers and leaves V's row count, and the least-recently-written choice
of the two posterior buffers across a save and restore. Then it walks every sequence of 1
to 4 of 16 calls (set_data to 0 / 5 / 8 rows, append of 0 / 3, predict, batch steps of 3 / 0
rows, truncate to 0 / 5 / 8, new hyperparameters, new grid, capacity growth, a failed
deferred status, a planner's loop), from a new model and from a predicted one, incremental
mode on and off: 4 x (16 + 256 + 4,096 + 65,536) = 279,616 sequences, the state's rules
(factor_N <= N when factored, no tag beyond N after rows_cut(N), res_find(n) >= 0 only for
a tag of the current generation) asserted on every prefix, next to a shadow of what the
launches wrote: no predicate a call acts on may name rows the shadow does not hold.
CPU only; the same life of a model on the GPU is tests/test_gpu_state_paths.py."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_state_events_predicates_and_walk(tmp_path):
    import __graft_entry__ as ge
    exe = tmp_path / "state_main"
    cxx = shutil.which("c++") or shutil.which("g++") or ge.HIPCC
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", ge.CSRC, os.path.join(HERE, "state_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=20)   # (the walk takes under 2 s)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
