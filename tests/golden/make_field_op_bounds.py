"""Writes tests/golden/field_op_bounds.json: for every case of tests/field_op_cases.py and every output or gradient tensor, [err32, errK, max|f64|]:
err32 = max|f32 - f64| of the REFERENCE formulation itself (the same restatement evaluated in float32 and in float64 on the CPU), errK = max|K - f64|
of the restatement's declared-arithmetic mode (the roundings the kernel headers declare: table softplus, bf16 splits, record rounding of the table
gradient).  No kernel of the project is involved, and no number here is read off a kernel's error.  tests/test_gpu_field_ops.py allows the kernels
FACTOR * max(err32, errK) + FLOOR * max|f64| per tensor (FACTOR, FLOOR: tests/step_op_cases.py).

    python tests/golden/make_field_op_bounds.py            (CPU only; one thread, so that float32 sums do not depend on the machine's core count)

"open": tensors that exceed their bound on an MI355X for a reason not settled yet, {family: {tensor: {"ratio": measured (err - floor) / max(err32,
errK), "cases": [...], "note": ...}}}; the GPU tier asserts those at the tolerance the suite applied before (2e-3 of max, 3e-4 for g_x).  Filled in
by hand from the GPU tier's printed figures (tests/golden/field_op_open.json), never silently."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import field_op_cases as FC          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "field_op_bounds.json")
OPEN = os.path.join(ROOT, "tests", "golden", "field_op_open.json")


def build():
    torch.set_num_threads(1)
    with open(OPEN) as f:
        doc = {"rule": {"factor": FC.FACTOR, "floor": FC.FLOOR, "gmax_min": FC.GMAX_MIN}, "open": json.load(f), "families": {}}
    for fam, (cases, evaluate, _) in FC.families().items():
        recs = {}
        for cid, c in cases.items():
            r64, r32, rK = evaluate(c, (torch.float64, torch.float32, FC.K))
            rec = {"tensors": FC.measure3(r32, rK, r64)}
            rec["gmax"] = rec["tensors"][FC.GMAX_KEY[fam]][2]
            assert rec["gmax"] >= FC.GMAX_MIN, f"{fam}/{cid}: max|g| = {rec['gmax']}: a degenerate gradient case"
            recs[cid] = rec
        doc["families"][fam] = recs
    return doc


def dumps(doc):
    return json.dumps(doc, indent=0, sort_keys=True, separators=(",", ":")) + "\n"


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(dumps(build()))
    print("wrote", OUT)
