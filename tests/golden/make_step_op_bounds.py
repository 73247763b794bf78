"""Writes tests/golden/step_op_bounds.json: for every case of tests/step_op_cases.py and every output or gradient tensor, the rounding error of the
REFERENCE formulation itself -- the same restatement evaluated once in float32 and once in float64 on the CPU: err32 = max|f32 - f64| and max|f64|.
No kernel of the project is involved.  tests/test_gpu_step_ops.py allows the kernels FACTOR * err32 + FLOOR * max|f64| per tensor.

    python tests/golden/make_step_op_bounds.py            (CPU only; one thread, so that float32 sums do not depend on the machine's core count)

Where a tensor of a case needs more than FACTOR, tests/golden/step_op_widened.json holds the measured ratio (kernel error - floor) / err32 of that
case, taken from the figures the GPU tier prints on an MI355X; the case is allowed the next power of two, and the reason per tensor is below
(DESIGN.md section 5.2).  Every other case keeps FACTOR."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import step_op_cases as SC          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "step_op_bounds.json")

MEASURED = os.path.join(ROOT, "tests", "golden", "step_op_widened.json")       # {family: {tensor: {case: ratio}}}

_CHAIN = ("the sigmoid arguments are (sdf -+ half) inv_s: every fp32 rounding of half = iter_cos delta / 2 is multiplied by inv_s delta / 2 on its way into "
          "d sigmoid, in torch's float32 as in the kernel; where a handful of entries set the maximum torch's err32 is a single draw of that error, and the "
          "kernel's draw (a 1.5-ulp sigmoid, the suffix sum formed as total - prefix) is larger")
_TABLE = ("d true_cos is multiplied by the derivative of the table softplus: the derivative of a cubic whose value is within 2.1e-9 on a segment of 1 / 400 "
          "is accurate to ~2e-5 (worst at a segment's end, where true_cos == 0 of the rows with gradient == 0 lies), not to fp32")
_SUM = ("one number per launch, a signed sum over every sample: in front of the surface both sigmoids are within 1e-4 of 1 and the fp32 factors 1 - pc, "
        "1 - nc of their derivatives keep three digits, ~1e-9 per sample; torch's err32 for this single entry is one draw, as low as 1e-8 of the value")
REASONS = {"composite": {"g_sdf": _CHAIN, "g_normal": _CHAIN + "; and the table softplus' derivative, see packed_shading", "g_inv_s": _SUM},
           "packed_shading": {"g_sdf16": _CHAIN, "g_gradient": _TABLE, "g_gradient_zero_rows": _TABLE, "g_inv_s": _SUM}}


def widened():
    with open(MEASURED) as f:
        measured = json.load(f)
    doc = {}
    for fam, tensors in measured.items():
        for name, cases in tensors.items():
            if cases:
                doc.setdefault(fam, {})[name] = {"reason": REASONS[fam][name],
                                                 "cases": {cid: {"ratio": r, "factor": max(8.0, 2.0 ** math.ceil(math.log2(r)))} for cid, r in sorted(cases.items())}}
    return doc


def build():
    torch.set_num_threads(1)
    doc = {"rule": {"factor": SC.FACTOR, "floor": SC.FLOOR, "gmax_min": SC.GMAX_MIN}, "widened": widened(), "families": {}}
    for fam, (cases, evaluate, is_grad) in SC.families().items():
        recs = {}
        for cid, c in cases.items():
            r64 = evaluate(c, torch.float64)
            rec = {"tensors": SC.measure(evaluate(c, torch.float32), r64)}
            if is_grad(c):
                gmax = max(rec["tensors"][k][1] for k in SC.GMAX_KEY[fam])
                assert gmax >= SC.GMAX_MIN, f"{fam}/{cid}: max|g| = {gmax}: a degenerate gradient case"
                rec["gmax"] = gmax
            recs[cid] = rec
        doc["families"][fam] = recs
    return doc


def dumps(doc):
    return json.dumps(doc, indent=0, sort_keys=True, separators=(",", ":")) + "\n"


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(dumps(build()))
    print("wrote", OUT)
