"""CPU: the host side of the coloured mesh export -- geometry.save_ply byte for byte through a minimal reader, the loud refusal of CPU tensors / CPU models,
and the ctypes mirror of ac_mesh_attr_opts against the header (a C program prints the layout)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_ply(path):
    """-> (properties of the vertex element, vertex table, faces [F,3], total length): binary little-endian PLY with triangle faces only"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")[:-1]
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    counts, props, cur = {}, {}, None
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            cur = w[1]; counts[cur] = int(w[2]); props[cur] = []
        else:
            assert w[0] == "property"
            props[cur].append(" ".join(w[1:]))
    assert list(counts) == ["vertex", "face"] and props["face"] == ["list uchar int vertex_indices"]
    dt = np.dtype([(p.split()[1], {"float": "<f4", "uchar": "u1"}[p.split()[0]]) for p in props["vertex"]])
    nv, nf = counts["vertex"], counts["face"]
    vert = np.frombuffer(raw, dt, nv, end)
    face = np.frombuffer(raw, np.dtype([("n", "u1"), ("idx", "<i4", (3,))]), nf, end + nv * dt.itemsize)
    assert (face["n"] == 3).all()
    assert len(raw) == end + nv * dt.itemsize + nf * 13
    return props["vertex"], vert, face["idx"], len(raw)


def test_save_ply_round_trip(tmp_path):
    from avatarcraft_amd.geometry import save_ply
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.1, 0.2, 0.3]], np.float64)      # a tetrahedron + a loose vertex
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    n = (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1.0)).astype(np.float32)
    c = np.array([[0.0, 0.5, 1.0], [1.7, -0.2, 0.5], [0.25, 0.75, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], np.float32)
    xyz = ["float x", "float y", "float z"]; nrm = ["float nx", "float ny", "float nz"]; rgb = ["uchar red", "uchar green", "uchar blue"]
    for normals, colors, want_props, stride in ((None, None, xyz, 12), (n, None, xyz + nrm, 24), (None, c, xyz + rgb, 15), (n, c, xyz + nrm + rgb, 27)):
        path = tmp_path / f"m{stride}.ply"
        save_ply(str(path), v, t, normals=normals, colors=colors)
        props, vert, faces, size = read_ply(str(path))
        assert props == want_props and len(vert) == 5 and vert.dtype.itemsize == stride and np.array_equal(faces, t)
        header = open(path, "rb").read().index(b"end_header\n") + 11
        assert size == header + 5 * stride + 4 * 13
        assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), v.astype(np.float32))
        if normals is not None:
            assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), n)
        if colors is not None:
            got = np.stack([vert["red"], vert["green"], vert["blue"]], 1)
            assert got[0].tolist() == [0, 128, 255] and got[1].tolist() == [255, 0, 128] and got[2].tolist() == [64, 191, 255] and got[4].tolist() == [255] * 3
    # tensors (float64 vertices, int32 triangles, as extract_colored_mesh(return_torch=True) hands them over) write the same bytes
    save_ply(str(tmp_path / "t.ply"), torch.from_numpy(v), torch.from_numpy(t), normals=torch.from_numpy(n), colors=torch.from_numpy(c))
    assert open(tmp_path / "t.ply", "rb").read() == open(tmp_path / "m27.ply", "rb").read()


def test_cpu_tensors_and_cpu_models_are_refused(tmp_path):
    from avatarcraft_amd import nsr_ops, drivers
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        nsr_ops.mesh_vertex_attrs(None, torch.zeros(4, 3, dtype=torch.float64), 1.6)
    torch.manual_seed(0)
    net = NeRFNetwork()
    for colors in (True, False):
        with pytest.raises(RuntimeError, match="on the GPU"):
            net.extract_colored_mesh(1.6, 16, colors=colors)
    with pytest.raises(RuntimeError, match="on the GPU"):
        drivers.export_mesh(net, str(tmp_path / "never.ply"), resolution=16)
    assert not (tmp_path / "never.ply").exists()


def test_mesh_attr_opts_mirror_matches_the_header(tmp_path):
    from avatarcraft_amd import _lib
    fields = [f[0] for f in _lib.ac_mesh_attr_opts._fields_]
    assert fields == ["bound", "fd_eps", "target_sdf", "refine_steps", "tol", "max_move"]
    src = tmp_path / "layout.c"
    src.write_text('#include "avatarcraft_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%zu ' + " ".join(["%zu"] * len(fields)) + '\\n", sizeof(ac_mesh_attr_opts), '
                   + ", ".join(f"offsetof(ac_mesh_attr_opts, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True, timeout=60).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.ac_mesh_attr_opts) == 24
    assert out[1:] == [getattr(_lib.ac_mesh_attr_opts, f).offset for f in fields]
    assert _lib.ac_mesh_attr_opts.refine_steps.size == 4 and "ac_mesh_vertex_attrs" in _lib.EXPORTS
