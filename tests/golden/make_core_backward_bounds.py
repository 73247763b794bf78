"""Writes tests/golden/core_backward_bounds.json: for every family-A case of tests/core_backward_cases.py and every gradient tensor, [err32, errK,
max|f64|]: err32 = max|f32 - f64| of the restatement itself, errK = max|K - f64| of its declared-arithmetic mode, both on the CPU.  No kernel of the
project is involved, and no number here is read off a kernel's error.  tests/test_gpu_core_backward.py allows ac_render_core_backward
FACTOR * max(err32, errK) + FLOOR * max|f64| per tensor (FACTOR, FLOOR: tests/step_op_cases.py).  Family B's bounds are formed at test time.

    python tests/golden/make_core_backward_bounds.py       (CPU only; one thread, so that float32 sums do not depend on the machine's core count)

tests/golden/core_backward_measured.json holds what was read off the GPU tier's printed figures on an MI355X, by hand and never silently:
  "widened": {tensor: {case: ratio}}, ratio = (kernel error - floor) / max(err32, errK): the case is allowed the next power of two, for the arithmetic
             reason given per tensor below;
  "open":    {tensor: {case: ratio}}: not explained; asserted at the tolerance the suite applied before (3e-4 of max|f64|).  At most three pairs."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import core_backward_cases as CC          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "core_backward_bounds.json")
MEASURED = os.path.join(ROOT, "tests", "golden", "core_backward_measured.json")
MAX_OPEN = 3

_SUM = ("one number per ray, a signed sum over the ray's samples of d alpha / d inv_s terms that cancel: in front of the surface both sigmoids are within "
        "1e-4 of 1 and the fp32 factors 1 - pc, 1 - nc of their derivatives keep three digits; the restatement's err32 for this entry is a single draw of "
        "that error (tests/golden/make_step_op_bounds.py measured a median ratio of 11 on the compositor alone)")
_SDF_SUM = ("d b2[0] is the plain sum over the samples of the compositor's d sdf (core_mid_kernel adds it into column 0 of d sdf_out16, and the SDF backward "
            "sums the centre evaluation's upstream): it inherits that tensor's error -- every fp32 rounding of half = iter_cos delta / 2 is multiplied by "
            "inv_s delta / 2 on its way into d sigmoid (tests/golden/make_step_op_bounds.py widens d sdf itself up to 9.8) -- and is a signed sum of it; one ray "
            "of the case alone is 7.0 times off on this entry, with a d inv_s 2134 times off on that ray.  The restatement's own error is one draw: with torch summing "
            "on several threads max(err32, errK) of the same tensor is 9.6e-6 instead of 2.5e-6")
REASONS = {"g_inv_s": _SUM, "g_b2": _SDF_SUM}


def marks():
    with open(MEASURED) as f:
        m = json.load(f)
    wide = {name: {"reason": REASONS[name], "cases": {cid: {"ratio": r, "factor": max(8.0, 2.0 ** math.ceil(math.log2(r)))} for cid, r in sorted(cases.items())}}
            for name, cases in m["widened"].items() if cases}
    opened = {name: {"note": m["notes"][name], "cases": dict(sorted(cases.items()))} for name, cases in m["open"].items() if cases}
    assert sum(len(e["cases"]) for e in opened.values()) <= MAX_OPEN
    return wide, opened


def build():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _build()
    finally:
        torch.set_num_threads(threads)


def _build():
    wide, opened = marks()
    doc = {"rule": {"factor": CC.FACTOR, "floor": CC.FLOOR, "gmax_min": CC.GMAX_MIN, "legacy": CC.LEGACY}, "widened": wide, "open": opened, "cases": {}}
    for cid, c in CC.cases_a().items():
        r64, r32, rK = CC.eval_a(c, (torch.float64, torch.float32, CC.K))
        rec = {"tensors": CC.measure(r32, rK, r64)[2]}
        rec["gmax"] = rec["tensors"]["g_W1"][2]
        assert rec["gmax"] >= CC.GMAX_MIN, f"{cid}: max|g_W1| = {rec['gmax']}: a degenerate gradient case"
        doc["cases"][cid] = rec
    return doc


def dumps(doc):
    return json.dumps(doc, indent=0, sort_keys=True, separators=(",", ":")) + "\n"


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(dumps(build()))
    print("wrote", OUT)
