#!/usr/bin/env python3
"""Generate tests/golden/mesh_entry_rules.json: what each of the nine launching C entries of the mesh index kernels (marching cubes dense and streamed, connected
components with compaction, vertex clustering) answers to one broken argument -- the status code and the ac_last_error() text -- and what their five *_scratch
entries return, recorded WITHOUT a GPU at the commit before their scratch walks and shared refusals moved into one host header, so that the shared code can be
compared with it cell for cell (tests/test_mesh_entry_rules_host.py replays the file against the built library).

    python tests/golden/make_mesh_entry_rules.py         (on a checkout whose avatarcraft_amd/ is exactly the parent commit's, built, on a machine
                                                          without a GPU: it refuses otherwise)

A cell = one entry x one row of ROWS[entry]: every argument valid (host addresses that are never read) except the row's one violation.  Every row is a call
the entry refuses before any device work, so it touches no buffer and launches nothing; the generator asserts that each one IS refused.  The rows are the ones
tests/test_mesh_components_host.py, test_mesh_decimate_host.py and test_mesh_streamed_host.py list, plus the same rules on the dense marching-cubes entries.
"scratch" holds the sizes: the three mesh entries over SHAPES (V, T), the two marching-cubes entries over GRIDS.
"""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "mesh_entry_rules.json")
AC_ERR_BAD_ARG = 1
P = 4096                                    # a non-NULL address that nothing dereferences
V, T, NC = 1000, 2000, 7                    # the mesh of the valid call (NC: its components)
BIG = 2 ** 40                               # a scratch size no rule finds short

SHAPES = [(0, 0), (1, 0), (3, 1), (1024, 1024), (1025, 1), (1, 1025), (2049, 5), (97492, 194980), (1580000, 3160000), (2 ** 31 - 1, 2 ** 31 - 1),
          (2 ** 31, 0), (0, 2 ** 31)]
GRIDS = [(2, 2, 2), (3, 2, 2), (48, 48, 48), (66, 512, 512), (512, 512, 512), (1290, 1290, 1290), (1296, 1296, 1296), (1, 8, 8), (8, 1, 8), (8, 8, 1)]
MESH_SCRATCH = ("ac_mesh_components_scratch", "ac_mesh_compact_scratch", "ac_mesh_cluster_scratch")
GRID_SCRATCH = ("ac_marching_cubes_scratch", "ac_marching_cubes_slab_scratch")

_MC = {"volume_null": dict(vol=None), "scratch_null": dict(scratch=None), "scratch_short": dict(short=1), "nx_1": dict(nx=1), "ny_1": dict(ny=1), "nz_1": dict(nz=1),
       "points_2p31": dict(nx=2 ** 11, ny=2 ** 10, nz=2 ** 10, nbytes=BIG)}
_MC_EMIT = {"den_0": dict(den=0.0), "span_null": dict(span=None), "lo_null": dict(lo=None), "vertices_null": dict(v=None),
            "triangles_null": dict(t=None)}
_SLAB = {"n_2": dict(nx=2), "n_2_first": dict(nx=2, first=1), "n_2_last": dict(nx=2, last=1), "n_1_whole": dict(nx=1, first=1, last=1), "ny_1": dict(ny=1),
         "nz_1": dict(nz=1), "points_2p31": dict(nx=2 ** 11, ny=2 ** 10, nz=2 ** 10, nbytes=BIG), "window_null": dict(vol=None), "scratch_null": dict(scratch=None),
         "scratch_short": dict(short=1)}
_LIMITS = {"V_2p31": dict(V=2 ** 31, nbytes=BIG), "T_2p31": dict(T=2 ** 31, nbytes=BIG)}
_CP = dict({"triangles_null": dict(tris=None), "component_null": dict(comp=None), "keep_null": dict(keep=None), "scratch_null": dict(scratch=None)}, **_LIMITS,
           **{"scratch_short": dict(short=1), "C_above_V": dict(C=V + 1), "triangles_over_no_vertex": dict(V=0, T=5, C=0)})
_MCL = dict({"vertices_null": dict(verts=None), "triangles_null": dict(tris=None), "scratch_null": dict(scratch=None), "grid_null": dict(grid=False)}, **_LIMITS,
            **{"h_0": dict(h=0.0), "h_negative": dict(h=-1.0), "h_nan": dict(h=float("nan")), "h_inf": dict(h=float("inf")), "n0_0": dict(n=(0, 4, 4)),
               "n1_above": dict(n=(4, 2 ** 21 + 1, 4)), "n2_0": dict(n=(4, 4, 0)), "scratch_short": dict(short=1)})
ROWS = {
    "ac_marching_cubes_count": dict(_MC, counts_null=dict(counts=None)),
    "ac_marching_cubes_emit": dict(_MC, **_MC_EMIT),
    "ac_marching_cubes_slab_count": dict(_SLAB, counts_null=dict(counts=None)),
    "ac_marching_cubes_slab_emit": dict(_SLAB, **_MC_EMIT, x0_overflows=dict(x0=2 ** 32 - 3), first_x0_not_0=dict(first=1, x0=6)),
    "ac_mesh_components": dict({"triangles_null": dict(tris=None), "root_null": dict(root=None), "component_null": dict(comp=None), "sizes_null": dict(sizes=None),
                                "counts_null": dict(counts=None), "scratch_null": dict(scratch=None)}, **_LIMITS,
                               **{"scratch_short": dict(short=1), "triangles_over_no_vertex": dict(V=0, T=5)}),
    "ac_mesh_compact_count": dict(_CP, counts_null=dict(counts=None)),
    "ac_mesh_compact_emit": dict(_CP, n_kept_vertices_above_V=dict(nkv=V + 1), n_kept_triangles_above_T=dict(nkt=T + 1), vertex_map_null=dict(vmap=None),
                                 kept_vertices_null=dict(kv=None), triangles_out_null=dict(to=None), kept_triangles_null=dict(kt=None)),
    "ac_mesh_cluster_count": dict(_MCL, cluster_null=dict(cluster=None), counts_null=dict(counts=None)),
    "ac_mesh_cluster_emit": dict(_MCL, n_clusters_above_V=dict(nc=V + 1), n_kept_triangles_above_T=dict(nt=T + 1), leader_null=dict(leader=None),
                                 members_null=dict(members=None), positions_null=dict(positions=None), triangles_out_null=dict(to=None),
                                 kept_triangles_null=dict(kt=None)),
}
ENTRIES = GRID_SCRATCH[:1] + ("ac_marching_cubes_count", "ac_marching_cubes_emit") + GRID_SCRATCH[1:] + ("ac_marching_cubes_slab_count", "ac_marching_cubes_slab_emit",
          "ac_mesh_components_scratch", "ac_mesh_components", "ac_mesh_compact_scratch", "ac_mesh_compact_count", "ac_mesh_compact_emit", "ac_mesh_cluster_scratch",
          "ac_mesh_cluster_count", "ac_mesh_cluster_emit")


def _marching_cubes(L, lib, entry, vol=P, nx=4, ny=8, nz=8, first=0, last=0, scratch=P, nbytes=None, short=0, counts=P, x0=6, den=1.0, span=True, lo=True, v=P, nv=1,
                    t=P, nt=1):
    slab = "_slab_" in entry
    d3 = C.c_double * 3
    span, lo = d3(1.0, 1.0, 1.0) if span else None, d3(0.0, 0.0, 0.0) if lo else None
    if nbytes is None:
        nbytes = int((lib.ac_marching_cubes_slab_scratch if slab else lib.ac_marching_cubes_scratch)(4, 8, 8))
    head = (vol, nx, ny, nz, 0.0) + ((first, last) if slab else ()) + (scratch, nbytes - short)
    if entry.endswith("_count"):
        return getattr(lib, entry)(*head, counts, None)
    return getattr(lib, entry)(*head, *((x0, 0) if slab else ()), den, span, lo, v, nv, t, nt, None)


def _components(L, lib, entry, tris=P, T=T, V=V, root=P, comp=P, sizes=P, maxc=V, counts=P, scratch=P, nbytes=None, short=0):
    nbytes = int(lib.ac_mesh_components_scratch(1000, 2000)) if nbytes is None else nbytes
    return lib.ac_mesh_components(tris, T, V, root, comp, sizes, maxc, counts, scratch, nbytes - short, None)


def _compact(L, lib, entry, tris=P, T=T, V=V, comp=P, keep=P, C=NC, scratch=P, nbytes=None, short=0, counts=P, vmap=P, kv=P, nkv=10, to=P, kt=P, nkt=10):
    nbytes = int(lib.ac_mesh_compact_scratch(1000, 2000)) if nbytes is None else nbytes
    head = (tris, T, V, comp, keep, C, scratch, nbytes - short)
    if entry.endswith("_count"):
        return lib.ac_mesh_compact_count(*head, counts, None)
    return lib.ac_mesh_compact_emit(*head, vmap, kv, nkv, to, kt, nkt, None)


def _cluster(L, lib, entry, verts=P, V=V, tris=P, T=T, grid=True, h=1.0, n=(4, 4, 4), scratch=P, nbytes=None, short=0, cluster=P, counts=P, leader=P, members=P,
             positions=P, nc=10, to=P, kt=P, nt=10):
    nbytes = int(lib.ac_mesh_cluster_scratch(1000, 2000)) if nbytes is None else nbytes
    g = C.byref(L.ac_cluster_grid((C.c_double * 3)(0.0, 0.0, 0.0), h, (C.c_uint32 * 3)(*n))) if grid else None
    head = (verts, V, tris, T, g, scratch, nbytes - short)
    if entry.endswith("_count"):
        return lib.ac_mesh_cluster_count(*head, cluster, counts, None)
    return lib.ac_mesh_cluster_emit(*head, leader, members, positions, nc, to, kt, nt, None)


def call(L, entry, row):
    """-> [status, message] of one cell"""
    lib = L.lib()
    fn = _marching_cubes if "marching_cubes" in entry else _components if entry == "ac_mesh_components" else _compact if "compact" in entry else _cluster
    status = int(fn(L, lib, entry, **ROWS[entry][row]))
    return [status, lib.ac_last_error().decode() if status else ""]


def record_rows(L):
    return {e: {row: call(L, e, row) for row in rows} for e, rows in ROWS.items()}


def record_scratch(L):
    lib = L.lib()
    return {"shapes": [[v, t] + [int(getattr(lib, e)(v, t)) for e in MESH_SCRATCH] for v, t in SHAPES],
            "grids": [[nx, ny, nz] + [int(getattr(lib, e)(nx, ny, nz)) for e in GRID_SCRATCH] for nx, ny, nz in GRIDS]}


def main():
    git = lambda *a: subprocess.run(("git",) + a, cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    if git("status", "--porcelain", "--", "avatarcraft_amd"):
        sys.exit("avatarcraft_amd/ differs from HEAD: the fixture is recorded from a committed parent, never from a working tree")
    if os.path.exists("/dev/kfd"):
        sys.exit("this machine has a GPU: record without one (a row that a mistake here made valid would launch on addresses that are not device memory)")
    from avatarcraft_amd import _lib as L
    rows = record_rows(L)
    for e, r in rows.items():
        for row, (status, msg) in r.items():
            assert status == AC_ERR_BAD_ARG and msg, (e, row, status, msg)          # every row is a refusal before any launch
    doc = {"header": {"parent_commit": git("rev-parse", "HEAD"), "generator": "tests/golden/make_mesh_entry_rules.py", "mesh": [V, T, NC]},
           "entries": list(ENTRIES), "mesh_scratch": list(MESH_SCRATCH), "grid_scratch": list(GRID_SCRATCH), "rows": rows, "scratch": record_scratch(L)}
    with open(FIXTURE, "w") as f:                                          # one cell per line: a changed answer shows as a changed line
        f.write('{"header": %s,\n "entries": %s,\n "mesh_scratch": %s,\n "grid_scratch": %s,\n "rows": {' %
                tuple(json.dumps(doc[k]) for k in ("header", "entries", "mesh_scratch", "grid_scratch")))
        f.write(",".join('\n  "%s": {\n    %s}' % (e, ",\n    ".join('"%s": %s' % (k, json.dumps(v)) for k, v in r.items())) for e, r in rows.items()))
        f.write('},\n "scratch": {%s}}\n' % ",".join('\n  "%s": [\n    %s]' % (k, ",\n    ".join(json.dumps(v) for v in doc["scratch"][k])) for k in ("shapes", "grids")))
    assert json.load(open(FIXTURE)) == json.loads(json.dumps(doc))
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes:", sum(len(r) for r in rows.values()), "refused cells,", len(SHAPES), "shapes,", len(GRIDS), "grids")


if __name__ == "__main__":
    main()
