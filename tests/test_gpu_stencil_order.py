"""-m gpu: the issue order of the finite-difference stencil's gathers (field_stencil.hpp: stencil_levels).

The stencil issues the centre's and the +x / -x points' corners grouped by their (y, z) combination, so that gathers of one cache line leave back to
back.  That is instruction order only: every corner must still land in the register its interpolation reads.  Small renders (<= 64 rays, 16 + 16
samples) through ac_render_rays with the per-sample outputs on, every output and the 7 x 8 stencil features of every sample bit for bit against the
CPU oracle, on rays chosen for the cases where a wrong pairing of corner and register would show."""
import numpy as np
import pytest
import torch

from tests.common import load_golden, make_rays
from tests.gpu_common import device_field, oracle_field, assert_bitwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1.6
EPS = np.float32(0.005)                 # the renderer's finite-difference step at normal_epsilon_ratio = 0
T0, UP = 16, 16
FLOAT_KEYS = ["image", "weights_sum", "depth", "normal_map", "eik", "z_vals", "weights", "alpha", "color", "sdf", "gradient"]


@pytest.fixture(scope="module")
def env(oracle):
    assert torch.cuda.is_available(), "these tests need a GPU"
    p = load_golden("nsr_params.npz")
    f, table = device_field(p)
    of = oracle_field(p, table)
    return dict(p=p, f=f, table=table, of=of, O=oracle, inv_s=float(p["inv_s"]), scale=np.asarray(of.scale, np.float32))


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def stencil_points(pts):
    """[7, M, 3]: the centre and p +- eps e_k clamped to the cube, in the order the kernel evaluates them (+x, -x, +y, -y, +z, -z)"""
    b = np.float32(BOUND)
    out = np.repeat(pts[None].astype(np.float32), 7, axis=0)
    for e in range(1, 7):
        k, s = (e - 1) // 2, (EPS if (e - 1) % 2 == 0 else -EPS)
        out[e, :, k] = np.clip(pts[:, k] + s, -b, b)
    return out


def unit(q):
    b = np.float32(BOUND)
    return ((q + b) / (b + b)).astype(np.float32)


def cell(env, level, q):
    """integer cell coordinate of normalised coordinates q on a level, as the encoder computes it"""
    return np.floor(unit(q) * env["scale"][level] + np.float32(0.5)).astype(np.int64)


def coord_at_cell_boundary(env, level, m8, delta):
    """a coordinate whose grid position on `level` is 8 * m8 + delta cells"""
    s = float(env["scale"][level])
    return np.float32(((8.0 * m8 + delta - 0.5) / s) * 2.0 * BOUND - BOUND)


def decode_feat7(feat7, N, T):
    """ac_render_out.feat7 [N T / 16, 14, 64, 4] -> [7 evaluations, 16 levels, N T samples, 2 channels]: float k = 8 e + 2 j + channel of lane 16 g + n
    (sample n of the tile, level 4 j + g) sits in group k / 4, component k % 4"""
    tiles = N * T // 16
    f = feat7.cpu().numpy().reshape(tiles, 14, 64, 4).transpose(0, 1, 3, 2).reshape(tiles, 7, 4, 2, 4, 16)      # [tile, e, j, c, g, n]
    return f.transpose(1, 2, 4, 0, 5, 3).reshape(7, 16, tiles * 16, 2)


def render_and_compare(env, ro, rd):
    """one launch with every per-sample output against the oracle, bit for bit -> (gpu dict, stencil points [7, N T, 3])"""
    from avatarcraft_amd import nsr_ops
    N = ro.shape[0]
    assert N <= 64
    g = nsr_ops.render_rays(env["f"], t(ro), t(rd), T0, UP, BOUND, env["inv_s"], extras=True, debug_indices=True, train_extras=True)
    torch.cuda.synchronize()
    r = env["O"].render_rays(env["of"], ro, rd, T0, UP, BOUND, env["inv_s"])
    for k in FLOAT_KEYS:
        assert_bitwise(g[k], r[k], k)
    assert_bitwise(g["ss_inds"], r["ss_inds"], "ss_inds")
    assert_bitwise(g["sort_index"], r["sort_index"], "sort_index")
    assert_bitwise(g["gradient_error"].reshape(1), np.float32([r["gradient_error"]]), "gradient_error")
    # the stencil features: the oracle's hash encoding of the seven points of every sample
    pts = np.clip(g["pts"].cpu().numpy().reshape(-1, 3), -np.float32(BOUND), np.float32(BOUND))
    sp = stencil_points(pts)
    got = decode_feat7(g["feat7"], N, T0 + UP)
    for e in range(7):
        want, _, _ = env["O"].hash_encode_forward(unit(sp[e]), env["table"], env["p"]["offsets"], env["of"].S, env["of"].H)
        assert_bitwise(got[e], want, f"stencil features of evaluation {e}")
    assert float(np.abs(got).max()) > 0
    return g, sp


def axis_rays(env, a, deltas=(0.25, -0.25, 1.5, -1.5)):
    """rays parallel to the two other axes (and one along axis a itself) whose coordinate a sits `delta` cells from a multiple-of-8 cell boundary of level 15"""
    ro, rd = [], []
    others = [k for k in range(3) if k != a]
    for di, d in enumerate(others):
        o3 = [k for k in range(3) if k not in (a, d)][0]
        for mi, m8 in enumerate((129, 131)):                        # level-15 blocks a little off the centre of the cube
            for delta in deltas:
                for sgn in (1.0, -1.0):
                    o = np.zeros(3, np.float32); dd = np.zeros(3, np.float32)
                    o[a] = coord_at_cell_boundary(env, 15, m8, delta)
                    o[d] = -2.0 * sgn; dd[d] = sgn
                    o[o3] = 0.03 + 0.11 * mi - 0.07 * di
                    ro.append(o); rd.append(dd)
    for sgn in (1.0, -1.0):                                          # along axis a itself: the samples cross the block boundaries
        o = np.full(3, 0.05, np.float32); dd = np.zeros(3, np.float32)
        o[a] = -2.0 * sgn; dd[a] = sgn
        ro.append(o); rd.append(dd)
    return np.stack(ro), np.stack(rd)


@pytest.mark.parametrize("a", [0, 1, 2])
def test_axis_parallel_rays_through_a_fine_block_edge(env, a):
    """samples within eps of a multiple-of-8 cell boundary of level 15 along axis a (a = 0: the x-trio straddles two sectors and the -x point's cell
    lies below the centre's aligned block; a = 1, 2: the same geometry on the axes that are NOT grouped, against having reordered the wrong one)"""
    ro, rd = axis_rays(env, a)
    assert ro.shape[0] <= 64
    g, sp = render_and_compare(env, ro, rd)
    n_par = ro.shape[0] - 2                                          # the rays with a constant coordinate a
    T = T0 + UP
    blk = lambda e: cell(env, 15, sp[e][: n_par * T, a]) // 8
    below = blk(2 * a + 2) < blk(0)                                  # the minus point's cell is in the block below the centre's
    above = blk(2 * a + 1) > blk(0)
    assert below.any() and above.any() and (~below).any()
    assert float(((blk(0) == 129) | (blk(0) == 131) | (blk(0) == 128) | (blk(0) == 130)).mean()) == 1.0
    # eps spans more than one cell on the fine group and less than one on the coarse levels: both branches of the stencil ran
    assert float(EPS) / (2 * BOUND) * env["scale"][15] > 1.0 > float(EPS) / (2 * BOUND) * env["scale"][8]


def test_rays_grazing_the_cube_faces(env):
    """rays in and just inside the faces at +-bound: the offset points beyond the face are clamped onto it (their cell and weights differ from an unclamped
    point's, the centre's do not), on every axis and both signs"""
    ro, rd = [], []
    for a in range(3):
        d = (a + 1) % 3
        o3 = (a + 2) % 3
        for sgn in (1.0, -1.0):
            for inset in (0.0, 0.002, 0.004, 0.006):
                o = np.zeros(3, np.float32); dd = np.zeros(3, np.float32)
                o[a] = sgn * (BOUND - inset); o[d] = -2.0; dd[d] = 1.0; o[o3] = 0.1 * sgn
                ro.append(o); rd.append(dd)
    ro, rd = np.stack(ro), np.stack(rd)
    g, sp = render_and_compare(env, ro, rd)
    pts = sp[0]
    b = np.float32(BOUND)
    for a in range(3):
        plus_clamped = (pts[:, a] + EPS > b) & (sp[2 * a + 1][:, a] == b)
        minus_clamped = (pts[:, a] - EPS < -b) & (sp[2 * a + 2][:, a] == -b)
        assert plus_clamped.any() and minus_clamped.any()
    assert (np.abs(pts).max(axis=1) == b).any() and (np.abs(pts).max(axis=1) < b).any()


def test_oblique_bundle(env):
    ro, rd = make_rays(8, 8, dist=1.7, f=6.0, jitter_seed=7)
    g, _ = render_and_compare(env, ro, rd)
    assert float(g["weights_sum"].max()) > 0.5 and float(g["weights_sum"].min()) < 0.1


def test_half_table_kernel_equals_fp32_kernel_on_the_widened_table(env):
    """the H16 copy of the reordered code: the same bundle from the half table and, through the fp32 kernel, from the widened table -- bit for bit"""
    from avatarcraft_amd import nsr_ops
    from tests.test_gpu_half_table import field_like, widened, same_bits, all_keys
    ro0, rd0 = make_rays(8, 8, dist=1.7, f=6.0, jitter_seed=7)
    ro1, rd1 = axis_rays(env, 0)
    fw = field_like(env["f"], widened(env["table"]))
    for ro, rd in ((ro0, rd0), (ro1, rd1)):
        a = nsr_ops.render_rays(env["f"], t(ro), t(rd), T0, UP, BOUND, env["inv_s"], extras=True, debug_indices=True, table_dtype="half")
        b = nsr_ops.render_rays(fw, t(ro), t(rd), T0, UP, BOUND, env["inv_s"], extras=True, debug_indices=True)
        torch.cuda.synchronize()
        same_bits(a, b, all_keys(UP), "half table")
    assert float(a["sdf"].abs().max()) > 0
