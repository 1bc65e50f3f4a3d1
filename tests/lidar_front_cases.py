"""Case table of the LiDAR front end -- `bevf_voxelize_f32`, `bevf_scatter_voxels_f32`, `bevf_vfe_smallk_max_f32`,
`bevf_lidar_filter_pad_f32` -- shared by tests/test_lidar_front_host.py (CPU: every case has the property it is named for) and
tests/test_gpu_lidar_front_edges.py (MI355X: the kernels against the oracle on these cases).  DESIGN.md 4.2.

Deterministic builders only (`synth` counters and closed forms), no GPU.  Where a case depends on an exact cell its coordinates are
dyadic: range (0, 0, 0, gx, gy, gz) with voxel 1 and points at cell + 0.25 + j / 64, so the subtraction and the division are exact.

Also here: two restatements the host file pins and the GPU file uses --
  * `voxelize_by_sorting`: hard voxelisation through a stable argsort / np.unique, no loop over points (the oracle's dict loop is
    held against it on the small cases, so the yardstick itself is checked);
  * `filter_pad_ref`: the numpy range filter + pad with a range argument and the out-of-range-choice rule of the kernel.
"""
import functools

import numpy as np
import torch

from bevfusion_multimodal_3d_object_detection_amd import synth
from bevfusion_multimodal_3d_object_detection_amd.encoders import DEFAULT_PC_RANGE, pillar_grid, sparse_grid

F32 = np.float32
PILLAR_VS = pillar_grid(DEFAULT_PC_RANGE, 50, 50)[4]                 # (2.048, 2.048, 8.0) in fp32


# ---- restatements ------------------------------------------------------------------------------------------------------------------

def grid_of(pc_range, voxel_size):
    """(gx, gy, gz) as the oracle sizes it, and the fp32 ratios it rounds."""
    lo, hi, vs = np.asarray(pc_range[:3], F32), np.asarray(pc_range[3:], F32), np.asarray(voxel_size, F32)
    ratio = (hi - lo) / vs
    return tuple(int(g) for g in np.round(ratio).astype(np.int64)), ratio


def cell_ids(pts, pc_range, voxel_size):
    """pts (N, C) fp32 -> (int64 cell id (z gy + y) gx + x, valid mask), the fp32 arithmetic of the oracle and the kernel."""
    (gx, gy, gz), _ = grid_of(pc_range, voxel_size)
    lo, vs = np.asarray(pc_range[:3], F32), np.asarray(voxel_size, F32)
    with np.errstate(invalid="ignore"):
        c = np.floor((pts[:, :3].astype(F32) - lo) / vs)
        ok = np.all((c >= 0) & (c < np.asarray([gx, gy, gz], F32)), axis=1)
    ci = np.where(ok[:, None], c, 0).astype(np.int64)
    return (ci[:, 2] * gy + ci[:, 1]) * gx + ci[:, 0], ok


def radix_passes(ncells: int) -> int:
    """8-bit digits needed to order cells 0 .. ncells - 1 AND keep the all-ones invalid cell behind them: the smallest p <= 4
    with 256^p > ncells."""
    p = 1
    while p < 4 and 256 ** p <= ncells:
        p += 1
    return p


def voxelize_by_sorting(points: torch.Tensor, pc_range, voxel_size, max_points: int, max_voxels: int):
    """Hard voxelisation without a loop over points: np.unique gives each cell's first point, the rank of that first point numbers
    the voxels, a stable argsort on the voxel number groups the points in input order.  Same outputs as `hard_voxelize`."""
    pts = points.numpy().astype(F32)
    B, N, C = pts.shape
    feats = np.zeros((B, max_voxels, max_points, C), F32)
    coords = np.zeros((B, max_voxels, 3), np.int64)
    npts = np.zeros((B, max_voxels), np.int32)
    nvox = np.zeros(B, np.int32)
    (gx, gy, gz), _ = grid_of(pc_range, voxel_size)
    for b in range(B):
        cid, ok = cell_ids(pts[b], pc_range, voxel_size)
        idx = np.nonzero(ok)[0]
        if idx.size == 0:
            continue
        uniq, first, inv = np.unique(cid[idx], return_index=True, return_inverse=True)
        rank = np.empty(uniq.size, np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(uniq.size)         # voxel number = order of first appearance
        vid = rank[inv.reshape(-1)]
        order = np.argsort(vid, kind="stable")                                # points grouped by voxel, input order inside
        vs_, ns = vid[order], idx[order]
        start = np.searchsorted(vs_, vs_, side="left")
        slot = np.arange(vs_.size) - start
        keep = (vs_ < max_voxels) & (slot < max_points)
        feats[b, vs_[keep], slot[keep]] = pts[b, ns[keep]]
        nv = min(uniq.size, max_voxels)
        nvox[b] = nv
        cnt = np.bincount(vid, minlength=uniq.size)
        npts[b, :nv] = np.minimum(cnt[:nv], max_points)
        u = uniq[np.argsort(rank)][:nv]
        coords[b, :nv] = np.stack([u // (gx * gy), (u // gx) % gy, u % gx], 1)
    return torch.from_numpy(feats), torch.from_numpy(coords), torch.from_numpy(npts), torch.from_numpy(nvox)


def filter_pad_ref(points: np.ndarray, max_points: int, pc_range=DEFAULT_PC_RANGE, choice=None):
    """Range filter with strict inequalities in fp32 (NaN fails every comparison), survivors in order; `choice` is used only when
    at least max_points survive, and an entry outside [0, survivors) gives a zero row; otherwise the first max_points
    survivors, zero padded.  -> ((max_points, C) fp32, survivors)."""
    r = np.asarray(pc_range, F32)
    with np.errstate(invalid="ignore"):
        m = np.ones(points.shape[0], bool)
        for a in range(3):
            m &= (points[:, a] > r[a]) & (points[:, a] < r[a + 3])
    p = points[m]
    n = p.shape[0]
    out = np.zeros((max_points, points.shape[1]), F32)
    if choice is not None and n >= max_points:
        ch = np.asarray(choice, np.int64)
        ok = (ch >= 0) & (ch < n)
        out[ok] = p[ch[ok]]
    else:
        out[:min(n, max_points)] = p[:max_points]
    return out, n


# ---- voxeliser cases ---------------------------------------------------------------------------------------------------------------

def unit_range(gx, gy, gz=1):
    return (0.0, 0.0, 0.0, float(gx), float(gy), float(gz)), (1.0, 1.0, 1.0)


def points_in_cells(cells, grid, C, seed):
    """One fp32 point (C channels) per entry of `cells` (int64 id (z gy + y) gx + x; -1, -2, -3, -4 = out of range below x, above
    x, above y, below z): cell + 0.25 + j / 64 with j = point index mod 32, channel 3 = the point index, the rest U(0, 1)."""
    gx, gy, gz = grid
    cells = np.asarray(cells, np.int64)
    n = np.arange(cells.size)
    inside = cells >= 0
    c = np.where(inside, cells, 0)
    frac = 0.25 + (n % 32) / 64.0
    x, y, zc = c % gx + frac, (c // gx) % gy + frac, c // (gx * gy) + frac
    x = np.where(cells == -1, -0.5, np.where(cells == -2, gx + 0.5, x))
    y = np.where(cells == -3, gy + 0.5, y)
    zc = np.where(cells == -4, -0.5, zc)
    pts = synth.uniform((cells.size, C), seed).numpy().astype(F32)
    pts[:, 0], pts[:, 1], pts[:, 2] = x, y, zc
    if C > 3:
        pts[:, 3] = n
    return pts


def _case(pts, pc_range, vs, P, Nv):
    pts = np.asarray(pts, F32)
    if pts.ndim == 2:
        pts = pts[None]
    return dict(pts=torch.from_numpy(np.ascontiguousarray(pts)), pc_range=tuple(pc_range), vs=tuple(vs), P=P, Nv=Nv)


def _pass_boundary(gx, gy):
    """~3000 points: random cells with repeats, cell 0, the top cell, every reachable cell whose low one / two / three digits are
    all 0xFF, out-of-range points on three faces; top-cell and out-of-range points ALTERNATE (a sort that is one digit short leaves
    the invalid cell, all ones, among the top cell's keys and splits its segment)."""
    ncells = gx * gy
    rnd = synth.randint((2950,), 1000 + gx + gy, 0, ncells).numpy()
    rnd = rnd[synth.randint((2950,), 7, 0, 1300).numpy()] if ncells > 1300 else rnd      # repeats: segments longer than 1
    ff = [c for c in (0xFF, 0x1FF, 0xFFFF, 0x1FFFF, 0xFEFFFF, 0xFFFFFF - 256, 0xFFFFFE, 0x7FFFFF) if c < ncells]
    top = ncells - 1
    mix = [top, -1, top, -2, 0, -3, top, -1, 0, top, -2, top]
    cells = np.concatenate([rnd[:1000], mix, ff, rnd[1000:2000], ff, mix, [0, top], rnd[2000:], [-2, top, -1, 0]])
    rng, vs = unit_range(gx, gy)
    return _case(points_in_cells(cells, (gx, gy, 1), 4, 50 + gx), rng, vs, 5, 3000)


def _near32():
    g = 65535
    top = g * g - 1
    cells = np.concatenate([[top, 0, -1, top, 0x12345678, 0xFFFEFFFF, 0xFF00FF00, 0, -2, top, 0xFFFEFFFE],
                            synth.randint((500,), 77, 0, g * g).numpy(), [top, 0]])
    rng, vs = unit_range(g, g)
    return _case(points_in_cells(cells, (g, g, 1), 4, 78), rng, vs, 3, 600)


PROD_VS = (0.1, 0.1, 0.2)                                         # DEFAULT_PC_RANGE / (1024, 1024, 40)
PROD_N = 263205                                                   # 258 tiles of 1024: vox_vid's tile loop takes a second trip


def _prod4pass():
    _, pts, _ = synth.frame_inputs(1, 0, 0, 0, PROD_N, 4, seed=4242)
    pts = pts.clone()
    pts[0, 5::40000, :3] = pts[0, 5, :3]                            # seven points in one voxel, tiles apart: the point cap binds
    return _case(pts.numpy(), DEFAULT_PC_RANGE, PROD_VS, 2, 300000)


LONG_N = (1 << 20) - 1
LONG_GRID = (7, 5, 3)


def _longvec():
    """N = 2^20 - 1, C = 3, 105 cells that first appear all along the sweep (cell < 1 + 105 n / N), a third of the points out of
    range, and the last point alone in the last cell: heads in tiles past 256 and a head at the largest point index."""
    n = np.arange(LONG_N, dtype=np.int64)
    h = synth.randint((LONG_N,), 99, 0, 1 << 30).numpy()
    cells = h % (1 + (104 * n) // LONG_N)
    cells[h % 3 == 0] = -1 - (h[h % 3 == 0] >> 8) % 4
    cells[-1] = 104
    rng, vs = unit_range(*LONG_GRID)
    return _case(points_in_cells(cells, LONG_GRID, 3, 98), rng, vs, 4, 200)


def _tile_edge(N):
    _, pts, _ = synth.frame_inputs(1, 0, 0, 0, N, 4, seed=300 + N)
    return _case(pts.numpy(), DEFAULT_PC_RANGE, PILLAR_VS, 4, 700)


SINGLE_CELL = 37                                                  # of the 11 x 9 grid below


def _single(P):
    rng, vs = unit_range(11, 9)
    return _case(points_in_cells(np.full(5000, SINGLE_CELL), (11, 9, 1), 4, 60), rng, vs, P, 8)


SEG_LENGTHS = (1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 199, 200, 201)      # cell i holds SEG_LENGTHS[i] points


def _seglen(P):
    """Cells of 1 .. 201 points, interleaved: every cap of SINGLE_P meets a segment one shorter, equal and one longer."""
    cells = np.repeat(np.arange(len(SEG_LENGTHS)), SEG_LENGTHS)
    cells = cells[np.argsort(synth.uniform((cells.size,), 61).numpy(), kind="stable")]
    rng, vs = unit_range(5, 3)
    return _case(points_in_cells(cells, (5, 3, 1), 4, 62), rng, vs, P, 20)


SINGLE_P = (1, 63, 64, 65, 128, 200)
REVERSE_N = 3000


def _reverse(Nv):
    rng, vs = unit_range(64, 64)
    return _case(points_in_cells(np.arange(REVERSE_N)[::-1] + 500, (64, 64, 1), 4, 63), rng, vs, 3, Nv)


SEAM_GRID, SEAM_C, SEAM_N, SEAM_P = (40, 40, 1), 777, 2000, 16


def _seam(mirrored):
    """Frame 0: only valid points, cells <= c, 5 of them in c (fewer than the cap: the probe of c's segment runs on over the end of
    the frame).  Frame 1: cells >= c, 300 points in c, which is therefore its first sorted key.  Frame 2: nothing in range."""
    f0 = synth.randint((SEAM_N,), 64, 0, SEAM_C).numpy()
    f0[[3, 700, 701, 1500, SEAM_N - 1]] = SEAM_C
    f1 = synth.randint((SEAM_N,), 65, SEAM_C + 1, 1600).numpy()
    f1[synth.randint((300,), 66, 0, SEAM_N).numpy()] = SEAM_C
    f1[[0, 5, SEAM_N - 1]] = SEAM_C
    f1[10::97] = -2
    f2 = -1 - synth.randint((SEAM_N,), 67, 0, 4).numpy()
    frames = [points_in_cells(f, SEAM_GRID, 4, 68 + i) for i, f in enumerate((f0, f1, f2))]
    rng, vs = unit_range(*SEAM_GRID)
    return _case(np.stack(frames[::-1] if mirrored else frames), rng, vs, SEAM_P, 1700)


def _ulps(v, ks):
    out = []
    for k in ks:
        x = F32(v)
        for _ in range(abs(k)):
            x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
        out.append(x)
    return out


NUMERIC_DENORMAL = F32(-1e-40)


def _numeric_unit():
    """Range (0,0,0)-(4,4,4), voxel 1.  Per axis, the other two at 1.5: +-0.0 (cell 0, both), +-inf and NaN (dropped), -1e-40
    (floor -1: dropped; a flush-to-zero subtraction would put it in cell 0), +1.4e-45 (cell 0), one ulp on either side of the
    faces 0 and 4 and of the interior borders 1, 2, 3."""
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, NUMERIC_DENORMAL, F32(1e-45)]
    for border in (0.0, 1.0, 2.0, 3.0, 4.0):
        vals += _ulps(border, (-1, 0, 1))
    rows = []
    for axis in range(3):
        for v in vals:
            p = [1.5, 1.5, 1.5, float(len(rows))]
            p[axis] = v
            rows.append(p)
    return _case(np.asarray(rows, F32), (0, 0, 0, 4, 4, 4), (1, 1, 1), 8, 80)


def _numeric_pillar():
    """The 50 x 50 pillar grid: x and y within four ulps of every cell border k = 0 .. 50 (the faces included) and z of the two z
    faces.  Some quotients (x - x0) / vx lie below k and round onto it: the host file counts them."""
    lo, vs = np.asarray(DEFAULT_PC_RANGE[:3], F32), np.asarray(PILLAR_VS, F32)
    rows = []
    for axis in range(2):
        for k in range(51):
            for x in _ulps(lo[axis] + F32(k) * vs[axis], range(-4, 5)):
                p = [1.0, 1.0, 0.0, float(len(rows))]
                p[axis] = x
                rows.append(p)
    for z in _ulps(DEFAULT_PC_RANGE[2], range(-2, 3)) + _ulps(DEFAULT_PC_RANGE[5], range(-2, 3)):
        rows.append([1.0, 1.0, z, float(len(rows))])
    return _case(np.asarray(rows, F32), DEFAULT_PC_RANGE, PILLAR_VS, 12, 2500)


def _channels(C):
    _, pts, _ = synth.frame_inputs(2, 0, 0, 0, 2000, C, seed=400 + C)
    pts = pts.clone()
    pts[:, ::13, 1] = -60.0
    return _case(pts.numpy(), DEFAULT_PC_RANGE, (6.4, 6.4, 4.0), 3, 300)       # 16 x 16 x 2 cells, both caps bind


def _reuse(which):
    if which == "large":
        _, pts, _ = synth.frame_inputs(2, 0, 0, 0, 5000, 5, seed=500)
        return _case(pts.numpy(), DEFAULT_PC_RANGE, PILLAR_VS, 8, 600)
    _, pts, _ = synth.frame_inputs(1, 0, 0, 0, 700, 5, seed=501)
    return _case(pts.numpy(), DEFAULT_PC_RANGE, (51.2, 51.2, 8.0), 4, 100)


PASS_GRIDS = ((255, 1, 1), (16, 16, 2), (257, 1, 2), (255, 257, 2), (256, 256, 3), (65537, 1, 3), (4095, 4097, 3), (4096, 4096, 4))

# name -> (one-line property, builder)
VOXEL_CASES = {}
for _gx, _gy, _p in PASS_GRIDS:
    VOXEL_CASES[f"pass_{_gx}x{_gy}"] = (f"{_gx * _gy} cells: {_p} radix pass(es); cell 0, top cell, 0xFF digits, invalid points",
                                        functools.partial(_pass_boundary, _gx, _gy))
VOXEL_CASES["near32"] = ("65535 x 65535 cells (4 passes, top cell 0xFFFE0000): cell 0 and the top cell", _near32)
VOXEL_CASES["prod4pass"] = ("1024 x 1024 x 40 production grid, N = 263205 (258 tiles), ~262k voxels: heads in every tile", _prod4pass)
VOXEL_CASES["longvec"] = ("N = 2^20 - 1, C = 3, 105 cells first seen all along the sweep, head at the last point", _longvec)
for _n in (1, 1023, 1024, 1025):
    VOXEL_CASES[f"tile_N{_n}"] = (f"N = {_n}: one key, one short of a tile, a full tile, a tile and one key", functools.partial(_tile_edge, _n))
for _P in SINGLE_P:
    VOXEL_CASES[f"single_P{_P}"] = (f"5000 points in one cell, cap {_P}: one digit bin, one head, a segment over five tiles",
                                    functools.partial(_single, _P))
    VOXEL_CASES[f"seglen_P{_P}"] = (f"segments of 1 .. 201 points against cap {_P}: shorter, equal, longer", functools.partial(_seglen, _P))
VOXEL_CASES["reverse_Nv1000"] = ("3000 distinct cells in descending order, max_voxels 1000 binds", functools.partial(_reverse, 1000))
VOXEL_CASES["reverse_Nv1"] = ("3000 distinct cells in descending order, max_voxels 1", functools.partial(_reverse, 1))
VOXEL_CASES["seam"] = ("B = 3: frame 0 ends in cell c, frame 1 starts in cell c, frame 2 empty", functools.partial(_seam, False))
VOXEL_CASES["seam_mirrored"] = ("the seam frames in the order empty, c first, c last", functools.partial(_seam, True))
VOXEL_CASES["numeric_unit"] = ("+-0, +-inf, NaN, denormals, one ulp around faces and borders, per axis", _numeric_unit)
VOXEL_CASES["numeric_pillar"] = ("50 x 50 pillars: within four ulps of every border; quotients that round onto an integer", _numeric_pillar)
for _C in (3, 5, 7, 16):
    VOXEL_CASES[f"channels_C{_C}"] = (f"C = {_C}, B = 2, 16 x 16 x 2 cells, both caps bind", functools.partial(_channels, _C))
VOXEL_CASES["reuse_large"] = ("first call into sentinel-filled out= buffers", functools.partial(_reuse, "large"))
VOXEL_CASES["reuse_small"] = ("second call, smaller in every dimension, into the same buffers", functools.partial(_reuse, "small"))

# the cases small enough for the second restatement and the host property checks to run in well under a second each
VOXEL_SMALL = [n for n in VOXEL_CASES if n not in ("prod4pass", "longvec")]


@functools.lru_cache(maxsize=None)
def voxel_case(name):
    return VOXEL_CASES[name][1]()


@functools.lru_cache(maxsize=None)
def voxel_oracle(name):
    """The oracle's outputs for a case, computed once per process and never modified by a test."""
    from oracle import ref_voxelize
    c = voxel_case(name)
    return ref_voxelize.hard_voxelize(c["pts"], c["pc_range"], c["vs"], c["P"], c["Nv"])


# grids the entry point must refuse: (pc_range, voxel_size, axis named in the message)
REFUSED_RATIOS = (((0, 0, 0, 5, 1, 1), (2, 1, 1), "x"),                      # 2.5: lroundf 3, np.round 2
                  ((0, 0, 0, 1, 49.4, 1), (1, 1, 1), "y"),
                  ((0, 0, 0, 1, 1, 49.4), (1, 1, 1), "z"))
ACCEPTED_BEV = (50, 128, 200)                                                # pillar and sparse (z_voxels 40) grids


def engine_grids(bev):
    """(pc_range, voxel_size, grid) of the pillar and the sparse-voxel encoder at bev x bev."""
    (D, H, W), svs = sparse_grid(DEFAULT_PC_RANGE, bev, bev, 40)
    return ((DEFAULT_PC_RANGE, pillar_grid(DEFAULT_PC_RANGE, bev, bev)[4], (bev, bev, 1)), (DEFAULT_PC_RANGE, svs, (W, H, D)))


# ---- scatter cases -----------------------------------------------------------------------------------------------------------------

OOB = (1 << 32, -1, None, 1 << 31, (1 << 32) + 3, -(1 << 32), (1 << 32) + 1)     # None = the axis' own size D


def _scatter(grid, B, Nv, C, kind, seed):
    D, H, W = grid
    feats = synth.normal((B, Nv, C), seed)
    coords = torch.stack([synth.randint((B, Nv), seed + 1, 0, D), synth.randint((B, Nv), seed + 2, 0, H),
                          synth.randint((B, Nv), seed + 3, 0, W)], 2)
    nv = None
    if kind == "one_cell":
        coords[:] = torch.tensor([D - 1, H // 2, W // 3])
    elif kind == "nv_zero":
        nv = torch.tensor(([0, min(17, Nv), Nv] * B)[:B], dtype=torch.int32)
    elif kind == "oob":                        # every listed value on every axis, the other two axes valid, in the LAST rows (a value
        r = 0                                  # that wrapped into the grid would win its cell); the rows before them random
        for axis in range(3):
            for v in OOB:
                coords[:, Nv - 1 - r, axis] = grid[axis] if v is None else v
                r += 1
        nv = torch.full((B,), Nv, dtype=torch.int32)
    return dict(feats=feats, coords=coords, grid=grid, nv=nv)


# name -> (property, grid (D,H,W), B, Nv, C, kind)
SCATTER_CASES = {
    "one_cell": ("all 300 rows of each frame name one cell: the last row wins", (2, 8, 11), 2, 300, 33, "one_cell"),
    "nv_zero": ("num_voxels 0 in frame 0 (an all-zero canvas), 17 in frame 1", (2, 8, 11), 2, 40, 65, "nv_zero"),
    "nv_absent": ("no num_voxels: every row is written; 2 x 176 cells is no multiple of 256", (2, 8, 11), 2, 300, 1, "plain"),
    "oob": ("-1, D, 2^31, 2^32+3, -2^32, 2^32, 2^32+1 on each axis stay out (no 32-bit wrap)", (2, 8, 11), 2, 64, 33, "oob"),
    "oob_thin": ("the same on the (3, 1, 7) grid, 3 x 21 cells", (3, 1, 7), 3, 64, 1, "oob"),
    "unit_grid": ("1 x 1 x 1 grid: 50 rows on the only cell", (1, 1, 1), 1, 50, 65, "plain"),
    "unit_grid_oob": ("1 x 1 x 1 grid with the out-of-range values", (1, 1, 1), 2, 64, 33, "oob"),
    "thin": ("(3, 1, 7) grid, C = 65, Nv = 1", (3, 1, 7), 1, 1, 65, "plain"),
}


@functools.lru_cache(maxsize=None)
def scatter_case(name):
    _, grid, B, Nv, C, kind = SCATTER_CASES[name]
    return _scatter(grid, B, Nv, C, kind, 600 + 7 * list(SCATTER_CASES).index(name))


# ---- VFE cases ---------------------------------------------------------------------------------------------------------------------
# The issue's cross is K = 1..16 x P in {1, PC-1, PC, PC+1, 2PC+1} (PC = 64 // K) x Cout in {1, 63, 64, 65, 132}.  In the kernel K
# (template) and P (the chunk loop, `np`, the readlane index) interact; Cout only sets the trips of the outer channel loop and the
# `live` mask, which gate nothing but the weight loads and the store.  Kept: every K with every distinct P of its set at Cout 64
# (bitwise against the two kernels) and 65 (a full chunk, then one live lane); Cout 1, 63, 132 at K = 4 (no dead lanes) and K = 7
# (dead lanes) with P = PC + 1.  Pruned: Cout 1, 63, 132 at the other fourteen K and the other P.

def vfe_points(K):
    pc = 64 // K
    return sorted({p for p in (1, pc - 1, pc, pc + 1, 2 * pc + 1) if p >= 1})


VFE_G = 9                                                          # three workgroups, the last with one live wave
VFE_COUT_EDGE = [(K, 64 // K + 1, c) for K in (4, 7) for c in (1, 63, 132)]
VFE_BIG = (32771, 2, 4, 8)                                         # G past the 8192-block cap: three voxels on the second trip


def vfe_inputs(G, P, K, Cout, seed, kind="plain"):
    x = synth.normal((G, P, K), seed)
    w = synth.normal((Cout, K), seed + 1, 0, 0.5)
    sc, sh = synth.uniform((Cout,), seed + 2, 0.5, 1.5), synth.normal((Cout,), seed + 3, 0, 0.3)
    if kind == "nan":
        x[0, 0, 0] = float("nan")
        x[G - 1, P - 1, K - 1] = float("nan")
    elif kind == "zero_row":
        x[:, P - 1] = 0.0
        x[1] = 0.0
    elif kind == "negative":                   # x > 0, w < 0, shift < 0, scale > 0: every pre-activation is negative
        x, w, sh = x.abs() + 0.1, -w.abs() - 0.1, -sh.abs() - 0.1
    elif kind == "no_affine":
        sc = sh = None
    return x, w, sc, sh


def vfe_ref(x, w, sc, sh):
    """fp64: (max_p relu((x . w) scale + shift), the same on absolute values without the relu).  A NaN pre-activation is 0 after
    the kernel's `!(v > 0) ? 0 : v` and contributes nothing to the bound."""
    x, w = x.double(), w.double()
    sc = torch.ones(w.shape[0], dtype=torch.float64) if sc is None else sc.double()
    sh = torch.zeros(w.shape[0], dtype=torch.float64) if sh is None else sh.double()
    v = torch.einsum("gpk,ck->gpc", x, w) * sc + sh
    b = torch.einsum("gpk,ck->gpc", x.abs(), w.abs()) * sc.abs() + sh.abs()
    v = torch.where(v > 0, v, torch.zeros_like(v))
    return v.amax(1), torch.nan_to_num(b, nan=0.0).amax(1)


# ---- filter / pad cases ------------------------------------------------------------------------------------------------------------

FILTER_BIG_N = (1 << 20) + 1029                                    # 1026 tiles: tile 1025 adds its 1025 counts in two trips
UNIT_BOX = (0.0, 0.0, 0.0, 4.0, 4.0, 4.0)
POISON = 777.0                                                     # what the GPU test leaves in `work` behind the survivors


def _sweep(N, C, seed):
    _, pts, _ = synth.frame_inputs(1, 0, 0, 0, max(N, 1), C, seed=seed)
    p = pts[0, :N].numpy().copy()
    p[::7, 0] *= 1.3                                               # some outside
    p[3::11, 2] -= 4.0
    return p


def _filter_case(points, max_points, pc_range=DEFAULT_PC_RANGE, choice=None):
    return dict(pts=np.ascontiguousarray(points, F32), max_points=max_points, pc_range=tuple(pc_range),
                choice=None if choice is None else np.asarray(choice, np.int64))


def _filter_big():
    p = np.full((FILTER_BIG_N, 3), 100.0, F32)                     # one point in 64 inside, the very last one too
    n = np.arange(0, FILTER_BIG_N, 64)
    p[n] = np.stack([(n % 97) * 0.5 - 20.0, (n % 89) * 0.5 - 20.0, (n % 13) * 0.25 - 1.0], 1)
    p[-1] = (1.0, 2.0, 0.5)
    return _filter_case(p, 20000)


def _filter_numeric():
    vals = [0.0, -0.0, np.nan, np.inf, -np.inf, NUMERIC_DENORMAL, F32(1e-45)] + _ulps(0.0, (-1, 1)) + _ulps(4.0, (-1, 0, 1))
    rows = []
    for axis in range(3):
        for v in vals:
            p = [1.5, 1.5, 1.5, float(len(rows))]
            p[axis] = v
            rows.append(p)
    return _filter_case(np.asarray(rows, F32), 64, UNIT_BOX)


def _filter_faces():
    rows = []
    for axis in range(3):
        for face in (DEFAULT_PC_RANGE[axis], DEFAULT_PC_RANGE[axis + 3]):
            for x in _ulps(face, (-1, 0, 1)):
                p = [1.0, 1.0, 0.0, float(len(rows)), 0.5]
                p[axis] = x
                rows.append(p)
    return _filter_case(np.asarray(rows, F32), 32)


def _filter_choice(delta, bad=False):
    """300 points of which exactly 100 survive; max_points = 100 - delta.  bad: choice entries -1, count and 2^40 among valid ones."""
    p = np.full((300, 4), 90.0, F32)
    keep = np.arange(0, 300, 3)
    p[keep] = _sweep(100, 4, 720) * F32(0.5)
    p[:, 3] = np.arange(300)
    mp = 100 - delta
    ch = (np.arange(mp) * 37 + 5) % 100
    if bad:
        ch[[0, 7, 50, mp - 1]] = [-1, 100, 1 << 40, 100]
    return _filter_case(p, mp, choice=ch)


FILTER_CASES = {f"N{n}": (f"N = {n}, C = 4", functools.partial(lambda n: _filter_case(_sweep(n, 4, 700 + n), 600), n))
                for n in (0, 1, 1023, 1024, 1025)}
FILTER_CASES["big"] = ("N = 2^20 + 1029, C = 3: 1026 tiles, 16402 survivors below max_points, the last point kept", _filter_big)
for _C in (3, 5, 7):
    FILTER_CASES[f"C{_C}"] = (f"C = {_C}, N = 3000, survivors above max_points 1000, no choice: the first 1000",
                              functools.partial(lambda c: _filter_case(_sweep(3000, c, 710 + c), 1000), _C))
FILTER_CASES["all_kept"] = ("every point inside", lambda: _filter_case(_sweep(2500, 4, 715) * F32(0.5), 3000))
FILTER_CASES["none_kept"] = ("no point inside", lambda: _filter_case(_sweep(2500, 4, 716) + F32(200.0), 300))
FILTER_CASES["numeric"] = ("NaN, +-inf, +-0.0, denormals against a minimum of 0; one ulp around 0 and 4", _filter_numeric)
FILTER_CASES["faces"] = ("one ulp on either side of all six faces of the default range, C = 5", _filter_faces)
FILTER_CASES["choice_equal"] = ("choice, survivors == max_points: gathered", functools.partial(_filter_choice, 0))
FILTER_CASES["choice_fewer"] = ("choice, survivors == max_points - 1: the choice is ignored", functools.partial(_filter_choice, -1))
FILTER_CASES["choice_more"] = ("choice, survivors above max_points: gathered", functools.partial(_filter_choice, 30))
FILTER_CASES["choice_bad"] = ("choice entries -1, count and 2^40: zero rows", functools.partial(_filter_choice, 0, True))


@functools.lru_cache(maxsize=None)
def filter_case(name):
    return FILTER_CASES[name][1]()
