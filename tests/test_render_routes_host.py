"""The routing of NeRFNetwork's renders, without a GPU.

test_routes_equal_the_parent_commit: tests/golden/make_render_routes.py's record_all() -- every configuration of run() (the full product of the model's
switches), of the three step renders and of their background / noise draws, each launch recorded instead of made -- on the code as it is, compared entry
for entry with tests/golden/render_routes.json, which the same file recorded at the commit named in its header, before the routing became one function.

test_router_rows: instant_nsr.render_route called directly; the readable specification next to the exhaustive recording."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_render_routes", os.path.join(HERE, "golden", "make_render_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_routes_equal_the_parent_commit():
    G = _generator()
    with open(G.FIXTURE) as f:
        doc = json.load(f)
    assert len(doc["header"]["parent_commit"]) == 40
    assert (doc["header"]["rays"], doc["header"]["batch_size"], doc["header"]["bound"]) == (G.N_RAYS, G.BATCH, G.BOUND)
    assert {k: v["axes"] for k, v in doc["sets"].items()} == G.AXES          # the stored product is the generator's: nothing dropped on either side
    assert len(G.unpack(doc["sets"]["run"])) == 9 * 2 ** 9 * 3 * 3
    now = G.record_all()
    assert sorted(now) == sorted(doc["sets"])
    for name, stored in doc["sets"].items():
        then = G.unpack(stored)
        assert len(then) == len(now[name])
        for (cfg_then, out_then), (cfg_now, out_now) in zip(then, now[name]):
            assert cfg_then == cfg_now
            out_now = json.loads(json.dumps(out_now))                        # (tuples -> lists, as the file stores them)
            assert out_now == out_then, f"{name} {cfg_now}:\n  parent {out_then}\n  now    {out_now}"


ROUTER_DEFAULTS = dict(posed=False, needs_grad=False, full=True, training=False, near_far=False, per_sample=True, opacity_only=False,
                       fused_training="core", manual_backward=False, render_table_dtype="float", skip_masked_samples=False, posed_long_rays=False,
                       long_step_extras=False, use_viewdirs=False)


def _route(caller, num_steps, upsample_steps, **kw):
    from avatarcraft_amd.instant_nsr import render_route
    return render_route(caller, num_steps, upsample_steps, **dict(ROUTER_DEFAULTS, **kw))


def test_router_rows():
    from avatarcraft_amd.instant_nsr import Route
    # (caller, counts, what differs from the defaults) -> entry, the options that depend on the route, what follows the launch
    rows = [
        ("run", (64, 64), {},
         Route("render_rays", dict(extras=True, skip_masked=False, opacity_only=False, table_dtype="float"), None)),
        ("run", (64, 64), dict(render_table_dtype="half", per_sample=False, posed=True, skip_masked_samples=True),
         Route("render_rays", dict(extras=False, skip_masked=True, opacity_only=False, table_dtype="half"), None)),
        ("run", (64, 64), dict(render_table_dtype="half", training=True),                 # the half table is an eval-mode, no-grad option
         Route("render_rays", dict(extras=True, skip_masked=False, opacity_only=False, table_dtype="float"), None)),
        ("run", (128, 128), dict(opacity_only=True),                                       # opacity_only reaches the long renderer with the switch on only
         Route("render_rays_long", dict(extras=True, skip_masked=False, opacity_only=False), None)),
        ("run", (128, 128), dict(opacity_only=True, long_step_extras=True),
         Route("render_rays_long", dict(extras=True, skip_masked=False, opacity_only=True), None)),
        ("run", (100, 64), dict(posed=True, posed_long_rays=True, skip_masked_samples=True),
         Route("render_rays_long", dict(extras=True, skip_masked=True, opacity_only=False), None)),
        ("run", (64, 64), dict(needs_grad=True), Route("render_core", {}, "guard")),
        ("run", (64, 64), dict(needs_grad=True, near_far=True), Route("sample_rays", {}, "autograd")),      # a mesh-guided range: sampling + autograd
        ("run", (64, 64), dict(needs_grad=True, fused_training="ops"), Route("sample_rays", {}, "autograd")),
        ("run", (128, 128), dict(needs_grad=True), Route("sample_rays_long", {}, "autograd")),
        ("run", (64, 64), dict(full=False), Route("sample_rays", {}, "autograd")),
        ("run", (64, 64), dict(needs_grad=True, manual_backward=True),
         Route("render_rays", dict(extras=True, train_extras=True), "last_train")),
        ("run", (128, 128), dict(needs_grad=True, manual_backward=True, long_step_extras=True),
         Route("render_rays_long", dict(extras=True, train_extras=True, save_stencil=True), "last_train")),
        ("run", (100, 64), dict(needs_grad=True, manual_backward=True, long_step_extras=True),             # 16 does not divide 164: keeps re-gathering
         Route("render_rays_long", dict(extras=True, train_extras=True), "last_train")),
        ("step_pair", (64, 64), dict(training=True), Route("render_rays_pair", {}, "last_train")),
        ("step_pair", (128, 128), dict(training=True, long_step_extras=True), Route("render_rays_long_pair", dict(save_stencil=True), "last_train")),
        ("step_pair", (128, 128), dict(training=True),                                     # two launches: the options are the training copy's
         Route("render_rays_long", dict(extras=True, train_extras=True), "last_train")),
        ("view_nograd", (64, 64), dict(opacity_only=True), Route("render_rays", dict(extras=False, opacity_only=True), None)),
        ("view_nograd", (128, 128), dict(opacity_only=True), Route("render_rays_long", dict(extras=False), None)),
        ("view_nograd", (128, 128), dict(opacity_only=True, long_step_extras=True),
         Route("render_rays_long", dict(extras=False, opacity_only=True), None)),
        ("view_train", (256, 0), dict(training=True, long_step_extras=True),               # the whole view never keeps the stencil features
         Route("render_rays_long", dict(extras=True, train_extras=True), "last_train")),
    ]
    for caller, (ns, us), kw, want in rows:
        got = _route(caller, ns, us, **kw)
        assert got == want, (caller, ns, us, kw, got)
    r = _route("run", 64, 64)
    with pytest.raises(AttributeError):                                                    # a record, not a bag
        r.entry = "render_rays_long"


def test_router_names_the_rule_today_s_order_names():
    with pytest.raises(NotImplementedError, match=r"posed-space rendering supports .* \(got 128 \+ 128\)"):
        _route("run", 128, 128, posed=True, needs_grad=True)                               # ... not "posed-space training": the switch is asked first
    with pytest.raises(RuntimeError, match=r"render_rays_long: num_steps=100 upsample_steps=40 unsupported"):
        _route("run", 100, 40, render_table_dtype="half")                                  # the envelope before the table
    with pytest.raises(RuntimeError, match=r"render_table_dtype must be one of \('float', 'half'\), got 'bfloat16'"):
        _route("run", 128, 128, render_table_dtype="bfloat16", posed=True, posed_long_rays=True, needs_grad=True)
    with pytest.raises(NotImplementedError, match="fused renderer's window only"):
        _route("run", 128, 128, render_table_dtype="half", posed=True, posed_long_rays=True)       # the table before the posed rules
    with pytest.raises(NotImplementedError, match="posed-space training is built for the short window only"):
        _route("run", 128, 128, posed=True, posed_long_rays=True, needs_grad=True, opacity_only=True)
    with pytest.raises(NotImplementedError, match="^opacity_only is not supported by the long renderer$"):
        _route("run", 128, 128, posed=True, posed_long_rays=True, opacity_only=True)
    with pytest.raises(NotImplementedError, match="fused operator only"):
        _route("run", 64, 64, posed=True, needs_grad=True, fused_training="ops", full=False)       # ... before "built for the default NeRFNetwork"
    with pytest.raises(NotImplementedError, match="built for the default NeRFNetwork"):
        _route("run", 64, 64, posed=True, full=False)
