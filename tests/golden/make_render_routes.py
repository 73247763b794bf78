#!/usr/bin/env python3
"""Generate tests/golden/render_routes.json: which nsr_ops entry every render of NeRFNetwork launches, with which options, or which rule its error names --
recorded WITHOUT a GPU at the commit the routing refactor started from, so that the refactored routing can be compared with it entry for entry
(tests/test_render_routes_host.py runs record_all() of this file on the working tree).

    python tests/golden/make_render_routes.py            (on a checkout whose avatarcraft_amd/ is exactly the parent commit's: it refuses otherwise)

How a route is recorded (the technique of tests/test_half_table_host.py): a default NeRFNetwork on the CPU, `_field` / `_field_sdf_only` /
`weight_norm_all` stubbed, every nsr_ops entry replaced by a recorder.  One recorded entry = the configuration + either the entry called (its non-tensor
arguments by value, its tensor arguments as None or their shape) or the exception's type and full message.

Sets:
  run           NeRFNetwork.run(), the FULL product of RUN_AXES (41 472 configurations, nothing pruned); the recorder raises, i.e. one launch per entry.
  run_not_full  the same with a model the fused renderer does not cover (curvature term on: _fused_supported() False), counts x space x grad x mode.
  run_bg        run() with every form of bg_color (None, scalar, [3], [N,3]) on the routes that hand it on differently.
  steps         render_step_pair / render_view_nograd / render_view_train on a stand-in for "the default model on the GPU" (a parameterless subclass),
                counts x long_step_extras x training x opacity_only x use_viewdirs; the recorders RETURN small results here, so every launch of a route,
                the order of background and noise draws (torch.rand wrapped) and what the render leaves behind (_last_train, the pair's background cache)
                are part of the entry.  Background call k returns the value 10 + k, noise draw k the value k + 1: the first column of the launched `bg` /
                `noise` shows which draw landed in which rows.
  step_draws    the three step renders with every form of background (None, scalar, [3], [n,3], one cached tensor, None mixed with tensors) and a
                torch.rand that ignores `out=`.

To keep the file small enough to read, an outcome names the configuration's counts instead of repeating them: the num_steps / upsample_steps arguments
of a call, the second dimension of its noise and the counts quoted in an error message are stored as "ns" / "us" (symbolic(): each is asserted equal to
the configuration's value before it is replaced, so nothing is lost), and a tensor is written "5x3" for shape [5, 3], "5xns:10,10,11" with the first
column of its rows (terse()).  The file stores each set as its axes, the list of distinct outcomes and a tree
over the axes in the order listed: a node has one child per value of its axis, a child is an outcome's index where every configuration below it has
that outcome, else "n<k>" = nodes[k]; equal subtrees are stored once.  unpack() gives back the full (configuration, outcome) entries.
"""
import contextlib
import itertools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FIXTURE = os.path.join(HERE, "render_routes.json")

COUNTS = [[64, 64], [32, 32], [16, 112], [128, 128], [100, 64], [256, 0], [2, 496], [100, 40], [400, 128]]
BOOL = [False, True]
RUN_AXES = {"counts": COUNTS, "posed": BOOL, "grad": BOOL, "train": BOOL, "manual_backward": BOOL, "fused_training": ["core", "ops", False],
            "long_step_extras": BOOL, "posed_long_rays": BOOL, "render_table_dtype": ["float", "half", "bfloat16"], "skip_masked_samples": BOOL,
            "opacity_only": BOOL, "per_sample": BOOL}
RUN_NOT_FULL_AXES = {"counts": COUNTS, "posed": BOOL, "grad": BOOL, "train": BOOL}
RUN_BG_AXES = {"bg": ["none", "scalar", "vec3", "full"], "counts": [[64, 64], [128, 128]], "grad": BOOL, "manual_backward": BOOL,
               "fused_training": ["core", False]}
STEP_RENDERS = ["render_step_pair", "render_view_nograd", "render_view_train"]
STEP_AXES = {"render": STEP_RENDERS, "counts": COUNTS, "long_step_extras": BOOL, "train": BOOL, "opacity_only": BOOL, "use_viewdirs": BOOL}
STEP_DRAW_AXES = {"render": STEP_RENDERS, "counts": [[64, 64], [128, 128]],
                  "bg": ["none", "scalar", "vec3", "full", "const", "mixed"], "rand_honours_out": BOOL}

ENTRIES = ("render_rays", "render_rays_long", "render_rays_pair", "render_rays_long_pair", "render_core", "sample_rays", "sample_rays_long")
N_RAYS, BATCH, BOUND = 5, 2, 1.6


class _Launched(Exception):
    def __init__(self, record):
        super().__init__(record["entry"])
        self.record = record


def configs(axes):
    names = list(axes)
    for values in itertools.product(*axes.values()):
        yield dict(zip(names, values))


@contextlib.contextmanager
def patched(*triples):
    """setattr(obj, name, value) for every triple, undone on exit"""
    saved = [(o, n, o.__dict__[n] if n in o.__dict__ else None, n in o.__dict__) for o, n, _ in triples]
    try:
        for o, n, v in triples:
            setattr(o, n, v)
        yield
    finally:
        for o, n, old, had in saved:
            if had:
                setattr(o, n, old)
            else:
                delattr(o, n)


def summary(v, rows=False):
    """a call argument as data: tensors as their shape (rows: + the first column, for the tagged draws of the step renders)"""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, torch.Tensor):
        s = {"shape": list(v.shape)}
        if rows and v.dim() == 2:
            s["rows"] = [float(x) for x in v[:, 0]]
        return s
    if isinstance(v, (list, tuple)):
        return [summary(x, rows) for x in v]
    return type(v).__name__


def call_record(name, a, kw, rows=False):
    return {"entry": name, "args": [summary(x, rows) for x in a], "kwargs": {k: summary(x, rows) for k, x in sorted(kw.items())}}


COUNT_ARGS = {"render_rays": (3, 4), "render_rays_long": (3, 4), "sample_rays": (3, 4), "sample_rays_long": (3, 4), "render_rays_pair": (4, 5),
              "render_rays_long_pair": (4, 5), "render_core": (16, 17)}           # where an entry takes num_steps, upsample_steps
NOISE_ARG = {"render_rays_pair": 3, "render_rays_long_pair": 3, "render_core": 12}   # ... and its noise, where positional


def symbolic(o, ns, us):
    """the configuration's counts in a recorded call / message / log -> "ns", "us" (in place; asserted equal first)"""
    if isinstance(o, dict) and o.get("entry") in COUNT_ARGS:
        i, j = COUNT_ARGS[o["entry"]]
        assert o["args"][i] == ns and o["args"][j] == us, o
        o["args"][i], o["args"][j] = "ns", "us"
        noises = [o["kwargs"].get("noise"), o["kwargs"].get("noise2")] + [o["args"][k] for e, k in NOISE_ARG.items() if e == o["entry"]]
        for t in noises:
            if t is not None:
                assert t["shape"][1] == ns, o
                t["shape"][1] = "ns"
    elif isinstance(o, dict):
        if "message" in o:
            o["message"] = o["message"].replace(f"{ns} + {us}", "{ns} + {us}").replace(f"num_steps={ns} upsample_steps={us}", "num_steps={ns} upsample_steps={us}")
        for e in o.get("log", ()):
            symbolic(e, ns, us)
    elif isinstance(o, list) and o[0] == "rand":
        assert o[1][1] == ns, o
        o[1][1] = "ns"
    return o


def terse(o):
    """{"shape": [5, 3]} -> "5x3", with rows "5x3:10,10,11,11,12" """
    if isinstance(o, dict) and "shape" in o:
        return "x".join(map(str, o["shape"])) + (":" + ",".join("%g" % r for r in o["rows"]) if "rows" in o else "")
    if isinstance(o, dict):
        return {k: terse(v) for k, v in o.items()}
    return [terse(v) for v in o] if isinstance(o, (list, tuple)) else o


def outcome_of(fn):
    try:
        fn()
    except _Launched as e:
        return e.record
    except Exception as e:                                         # the rule an error names is part of the route
        return {"raises": type(e).__name__, "message": str(e)}
    raise AssertionError("the render returned without a launch")


def background(kind, k, n):
    if kind == "none" or (kind == "mixed" and k % 2 == 0):
        return None
    if kind == "scalar":
        return 10.0 + k
    if kind == "vec3":
        return torch.full((3,), 10.0 + k)
    return torch.full((n, 3), 10.0 + k)


# ------------------------------------------------------------------------------------------------ run()
def record_run_sets():
    from avatarcraft_amd import instant_nsr as M
    ops = M.nsr_ops

    def recorder(name):
        def f(*a, **kw):
            raise _Launched(call_record(name, a, kw))
        return f
    stubs = [(ops, name, recorder(name)) for name in ENTRIES]
    stubs += [(ops, "weight_norm_all", lambda layers: [None] * len(layers)), (M.NeRFNetwork, "_field", lambda self: None),
              (M.NeRFNetwork, "_field_sdf_only", lambda self: None)]
    torch.manual_seed(0)
    net = M.NeRFNetwork()
    ro = torch.zeros(1, N_RAYS, 3)
    rd = torch.zeros(1, N_RAYS, 3)
    rd[..., 2] = 1.0
    warp = ops.WarpMesh.__new__(ops.WarpMesh)                      # (run() hands it on; it reads none of its device state)
    warp.use_mesh_guide, warp.accel, warp.verts = True, None, None

    def one(cfg):
        ns, us = cfg["counts"]
        train = cfg.get("train", False)
        net.train(train)
        net._manual_backward = cfg.get("manual_backward", False)
        net.fused_training = cfg.get("fused_training", "core")
        net.long_step_extras = cfg.get("long_step_extras", False)
        net.posed_long_rays = cfg.get("posed_long_rays", False)
        net.render_table_dtype = cfg.get("render_table_dtype", "float")
        net.skip_masked_samples = cfg.get("skip_masked_samples", False)
        kw = dict(perturb_overwrite=train, per_sample=cfg.get("per_sample", True), opacity_only=cfg.get("opacity_only", False))
        if cfg.get("posed", False):
            kw.update(render_can=False, verts=warp)
        bg = background(cfg.get("bg", "none"), 0, N_RAYS)
        with torch.set_grad_enabled(cfg["grad"]):
            return terse(symbolic(outcome_of(lambda: net.run(ro, rd, ns, BOUND, us, bg, **kw)), ns, us))
    with patched(*stubs):
        res = {"run": [(c, one(c)) for c in configs(RUN_AXES)]}
        res["run_bg"] = [(c, one(c)) for c in configs(RUN_BG_AXES)]
        net.curvature_loss = True
        res["run_not_full"] = [(c, one(c)) for c in configs(RUN_NOT_FULL_AXES)]
    return res


# ------------------------------------------------------------------------------------------------ the three step renders
def record_step_sets():
    from avatarcraft_amd import instant_nsr as M
    import types
    ops = M.nsr_ops
    log = []

    class Out(dict):
        opts = None

    def result(n):
        return Out(image=torch.zeros(n, 3), weights_sum=torch.zeros(n), eik_res=torch.zeros(2), eik=torch.zeros(n, 2))

    def recorder(name, pair):
        def f(*a, **kw):
            log.append(call_record(name, a, kw, rows=True))
            n = a[1].shape[0]
            return (result(n), result(n)) if pair else result(n)
        return f

    def groups(eik, group_rays):
        log.append({"entry": "eikonal_groups", "args": [summary(eik), group_rays], "kwargs": {}})
        return torch.zeros(((eik.shape[0] + group_rays - 1) // group_rays, 2))

    class StepNet(M.NeRFNetwork):
        """'the default model on the GPU' without a GPU: no parameters, the predicates the step renders ask answered as a GPU model answers them"""
        encoder = types.SimpleNamespace(embeddings=types.SimpleNamespace(is_cuda=True))

        def __init__(self):
            torch.nn.Module.__init__(self)

        def _fused_supported(self, ignore_curvature=False):
            return True

        def _field(self):
            return None

        def forward_variance(self):
            return None

        def _guard_finite(self, gerr):
            log.append("guard_finite")
    real_rand = torch.rand
    state = {"honours_out": True, "draws": 0}

    def rand(*size, out=None, **kw):
        state["draws"] += 1
        shape = list(size[0]) if len(size) == 1 and not isinstance(size[0], int) else list(size)
        log.append(["rand", shape, out is not None])
        if out is not None and state["honours_out"]:
            return out.fill_(float(state["draws"]))
        return torch.full(shape, float(state["draws"]))
    stubs = [(ops, name, recorder(name, "pair" in name)) for name in ENTRIES] + [(ops, "eikonal_groups", groups), (torch, "rand", rand)]
    ro = torch.zeros(N_RAYS, 3)
    rd = torch.zeros(N_RAYS, 3)
    rd[:, 2] = 1.0
    const = torch.full((1, 3), 7.0)

    def one(cfg):
        ns, us = cfg["counts"]
        net = StepNet()
        net.train(cfg.get("train", True))
        net.long_step_extras = cfg.get("long_step_extras", False)
        net.use_viewdirs = cfg.get("use_viewdirs", False)
        kind = cfg.get("bg", "full")
        state.update(honours_out=cfg.get("rand_honours_out", True), draws=0)
        del log[:]
        calls = [0]

        def bkg(*a):                                               # bkg_fn() | bkg_fn(n) | draw_fn(k, n)
            k, calls[0] = calls[0], calls[0] + 1
            log.append(["background"] + list(a))
            return const if kind == "const" else background(kind, k, a[-1] if a else N_RAYS)
        if cfg["render"] == "render_step_pair":
            fn = lambda: net.render_step_pair(ro, rd, ns, us, BOUND, bkg)
        elif cfg["render"] == "render_view_nograd":
            fn = lambda: net.render_view_nograd(ro, rd, ns, us, BOUND, bkg, BATCH, opacity_only=cfg.get("opacity_only", False))
        else:
            fn = lambda: net.render_view_train(ro, rd, ns, us, BOUND, bkg, BATCH)
        rec = {}
        try:
            rec["returns"] = summary(fn())
        except Exception as e:
            rec.update(raises=type(e).__name__, message=str(e))
        rec["log"] = list(log)
        last = net.__dict__.get("_last_train")
        rec["left"] = {"last_train": None if last is None else [summary(x, rows=True) for x in last[1:4]],
                       "last_train_groups": summary(net.__dict__.get("_last_train_groups")), "pair_bg_cache": "_pair_bg_cache" in net.__dict__}
        return terse(symbolic(rec, ns, us))
    with patched(*stubs):
        assert torch.rand is rand and real_rand is not rand
        return {"steps": [(c, one(c)) for c in configs(STEP_AXES)], "step_draws": [(c, one(c)) for c in configs(STEP_DRAW_AXES)]}


AXES = {"run": RUN_AXES, "run_bg": RUN_BG_AXES, "run_not_full": RUN_NOT_FULL_AXES, "steps": STEP_AXES, "step_draws": STEP_DRAW_AXES}


def record_all():
    """{set name: [(configuration, outcome), ...]} of the code that is importable now"""
    res = record_run_sets()
    res.update(record_step_sets())
    for name, axes in AXES.items():
        assert [c for c, _ in res[name]] == list(configs(axes)), name
    return res


def pack(entries, axes):
    """[(configuration, outcome)] in product order -> (distinct outcomes, nodes, root): see the module docstring"""
    keys, outcomes, index = {}, [], []
    for _, o in entries:
        k = json.dumps(o, sort_keys=True)
        if k not in keys:
            keys[k] = len(outcomes)
            outcomes.append(json.loads(k))
        index.append(keys[k])
    sizes = [len(v) for v in axes.values()]
    nodes, seen = [], {}

    def build(lo, depth, size):
        if all(i == index[lo] for i in index[lo:lo + size]):
            return index[lo]
        size //= sizes[depth]
        node = tuple(build(lo + k * size, depth + 1, size) for k in range(sizes[depth]))
        if node not in seen:
            seen[node] = "n%d" % len(nodes)
            nodes.append(list(node))
        return seen[node]
    return outcomes, nodes, build(0, 0, len(index))


def unpack(stored):
    """one stored set -> [(configuration, outcome)]"""
    sizes = [len(v) for v in stored["axes"].values()]

    def leaves(child, depth):
        if isinstance(child, int):
            n = 1
            for k in sizes[depth:]:
                n *= k
            return [child] * n
        return [i for c in stored["nodes"][int(child[1:])] for i in leaves(c, depth + 1)]
    index = leaves(stored["root"], 0)
    cfgs = list(configs(stored["axes"]))
    assert len(cfgs) == len(index)
    return [(c, stored["outcomes"][i]) for c, i in zip(cfgs, index)]


def main():
    git = lambda *a: subprocess.run(("git",) + a, cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    if git("status", "--porcelain", "--", "avatarcraft_amd"):
        sys.exit("avatarcraft_amd/ differs from HEAD: the fixture is recorded from a committed parent, never from a working tree")
    doc = {"header": {"parent_commit": git("rev-parse", "HEAD"), "generator": "tests/golden/make_render_routes.py",
                      "rays": N_RAYS, "batch_size": BATCH, "bound": BOUND}, "sets": {}}
    for name, entries in record_all().items():
        outcomes, nodes, root = pack(entries, AXES[name])
        doc["sets"][name] = {"axes": AXES[name], "outcomes": outcomes, "nodes": nodes, "root": root}
        assert unpack(doc["sets"][name]) == [(c, json.loads(json.dumps(o))) for c, o in entries], name
        print(f"{name}: {len(entries)} configurations, {len(outcomes)} distinct outcomes, {len(nodes)} tree nodes")
    with open(FIXTURE, "w") as f:                                  # one outcome per line: a changed route shows as a changed line
        f.write('{"header": %s,\n "sets": {' % json.dumps(doc["header"]))
        for i, (name, s) in enumerate(doc["sets"].items()):
            f.write('%s\n  "%s": {"axes": %s,\n   "outcomes": [\n    %s],\n   "nodes": %s,\n   "root": %s}' % (
                "," if i else "", name, json.dumps(s["axes"]), ",\n    ".join(json.dumps(o, sort_keys=True) for o in s["outcomes"]),
                json.dumps(s["nodes"], separators=(",", ":")), json.dumps(s["root"])))
        f.write("}}\n")
    assert json.load(open(FIXTURE))["sets"].keys() == doc["sets"].keys()
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
