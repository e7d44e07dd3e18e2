"""Fixture of tests/test_layer_routes_gpu.py: the routes of every conv + ABN pair, the library calls of one training step and one
teacher forward, and the autograd node on either side of Conv1x1's row-count gate (needs the GPU; imports the recorders from the
test, so both read the code the same way).  layer_routes.json was written by this script at the commit in FRONT of the one that
retired the conv + ABN node's library arm: there every route still carried its ``fused`` flag, and the script asserted it true on
each of them while recording - no pair of the step ever took the arm that was removed.
usage: python tests/golden/make_layer_routes_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_layer_routes_gpu as T     # noqa: E402

seen = {"routes": 0, "with_flag": 0}


def on_route(r):
    if r is not None:
        seen["routes"] += 1
        if hasattr(r, "fused"):
            seen["with_flag"] += 1
            assert r.fused, r


out = T.record_step(on_route)
again = T.record_step(on_route)
assert json.dumps(out) == json.dumps(again), "two recordings of the same step differ"
out["gate"] = T.record_gate()
with open(T.FIXTURE, "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
print("wrote", os.path.basename(T.FIXTURE), {k: len(v) for k, v in out.items()}, "routes taken", seen["routes"],
      "of them with a fused flag, all true:", seen["with_flag"], "gate", out["gate"])
