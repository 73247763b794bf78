#!/usr/bin/env python3
"""Compare the device code of two csrc trees kernel by kernel, on the CPU (hipcc cross-compiles; no GPU needed).

    python tools/isa_compare.py <parent csrc dir> <new csrc dir> [source.hip ...]

Every listed source (default: everything in build.SOURCES that exists in either tree) is compiled in both trees with avatarcraft_amd/build.py's FLAGS, its
PER_FILE_FLAGS and `--cuda-device-only -S`; the sources of build.VARIANTS (rec12: hash_stencil.hip with -DAC_REC8=0) once more with the variant's defines.
The assembly is cut at the function labels (label .. .Lfunc_end); comments, empty lines and the __hip_cuid_* lines (a hash of the source text) are dropped
and the basic-block labels .LBB<n>_ normalised; what is left is compared line for line.  One row per kernel: lines parent / now, .vgpr_count parent / now,
SAME or differs; a kernel that only one side has gets a row too.  Exit status 1 unless every row is SAME.  Each csrc directory must sit in a tree that has
include/avatarcraft_hip.h two levels up, as in the repository (a `git archive` of the parent commit unpacked beside the work tree does).
At most MAX_JOBS compilers run at once (default 16).
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from avatarcraft_amd import build  # noqa: E402

_LBB = re.compile(r"\.LBB\d+_")


def compile_asm(job):
    src, extra, out = job
    hipcc, flags = build._hipcc(), build.PER_FILE_FLAGS.get(os.path.basename(src), [])
    cmd = [hipcc] + build.FLAGS + (flags if build._supported(hipcc, flags) else []) + extra + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}")
    return out


def kernels_of(path):
    """{function name: (normalised lines, .vgpr_count or None)} of one assembly listing"""
    bodies, vgprs, names = {}, {}, set()
    cur = sym = None
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].rstrip()
            s = line.strip()
            if s.startswith(".type") and s.endswith(",@function"):
                names.add(s[len(".type"):].split(",")[0].strip())
            elif s.startswith(".symbol:"):                      # .amdgpu_metadata: .symbol precedes .vgpr_count within a kernel's entry
                sym = s.split(":", 1)[1].strip().strip("'\"")
                sym = sym[:-3] if sym.endswith(".kd") else sym
            elif s.startswith(".vgpr_count:") and sym:
                vgprs[sym] = int(s.split(":", 1)[1])
            if cur is None:
                if s.endswith(":") and s[:-1] in names:
                    cur = s[:-1]
                    bodies[cur] = []
                continue
            if s.startswith(".Lfunc_end"):
                cur = None
            elif s and "__hip_cuid_" not in s:
                bodies[cur].append(_LBB.sub(".LBB_", s))
    return {k: (v, vgprs.get(k)) for k, v in bodies.items()}


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    trees = [os.path.abspath(argv[1]), os.path.abspath(argv[2])]
    sources = argv[3:] or [s for s in build.SOURCES if any(os.path.exists(os.path.join(t, s)) for t in trees)]
    units = [(s, "", []) for s in sources]
    for name, per_src in build.VARIANTS.items():
        units += [(s, f" [{name}]", per_src[s]) for s in sources if s in per_src]
    try:
        workers = max(1, int(os.environ.get("MAX_JOBS", "16")))
    except ValueError:
        workers = 16
    with tempfile.TemporaryDirectory() as td:
        jobs = {}
        for u, (s, tag, extra) in enumerate(units):
            for side, t in enumerate(trees):
                if os.path.exists(os.path.join(t, s)):
                    jobs[(u, side)] = (os.path.join(t, s), extra, os.path.join(td, f"{u}_{side}.s"))
        with ThreadPoolExecutor(max_workers=workers) as ex:
            list(ex.map(compile_asm, jobs.values()))
        bad = 0
        print(f"{'translation unit':<28} {'lines parent':>12} {'lines now':>10} {'vgpr parent':>12} {'vgpr now':>9}  verdict       kernel")
        for u, (s, tag, extra) in enumerate(units):
            sides = [kernels_of(jobs[(u, side)][2]) if (u, side) in jobs else {} for side in (0, 1)]
            for k in list(sides[0]) + [k for k in sides[1] if k not in sides[0]]:
                p, n = sides[0].get(k), sides[1].get(k)
                if p is None or n is None:
                    verdict = "parent only" if n is None else "new only"
                else:
                    verdict = "SAME" if p == n else "differs"
                bad += verdict != "SAME"
                cell = lambda x, i: "-" if x is None or x[i] is None else (len(x[0]) if i == 0 else x[1])
                print(f"{s + tag:<28} {cell(p, 0):>12} {cell(n, 0):>10} {cell(p, 1):>12} {cell(n, 1):>9}  {verdict:<12}  {k}")
    print(f"{bad} row(s) not SAME" if bad else "every kernel SAME")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
