"""numpy restatement of the multi-sweep LiDAR merge and the pose chain (csrc/sweeps.hip), an independent plain
formulation of both, and the scenes tests/test_sweeps_host.py and tests/test_gpu_sweeps.py share.

The restatement does the device's operations in the device's order (four fp64 products and three sums per coordinate, written out as
scalar expressions on arrays, never `@`: BLAS may fuse), so the device output has to equal it bit for bit.  The plain formulation uses
np.linalg.inv, `@`, boolean masks and concatenate; the two agree on scenes whose points keep a margin from every decision boundary."""
import numpy as np

RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
MARGIN = 1e-3
INTERIOR = (7.5, -6.25, 0.5)                     # replaces a point that comes too close to a decision boundary


# ---- restatement: merge ------------------------------------------------------------------------------------------------------------

def transform_ref(T: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """(n, >=3) fp32 through the top 3 x 4 of the fp64 T, in fp64 in the device's order, not yet rounded: (n, 3) float64."""
    x, y, z = (pts[:, c].astype(np.float64) for c in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], 1)


def keep_ref(T: np.ndarray, pts: np.ndarray, close_radius: float, rng=RANGE):
    """(keep mask, transformed fp32 xyz) of one sweep's valid rows: close-point test on the sweep's own fp32 coordinates, strict range
    test on the rounded transformed ones (a NaN fails it)."""
    r = np.float32(close_radius)
    with np.errstate(invalid="ignore", over="ignore"):
        q = transform_ref(T, pts).astype(np.float32)
        close = (np.abs(pts[:, 0]) < r) & (np.abs(pts[:, 1]) < r) if r > 0 else np.zeros(len(pts), dtype=bool)
        lo, hi = np.array(rng[:3], dtype=np.float32), np.array(rng[3:], dtype=np.float32)
        inside = ((q > lo) & (q < hi)).all(1)
    return inside & ~close, q


def merge_ref(points: np.ndarray, counts: np.ndarray, T: np.ndarray, lag: np.ndarray, max_points: int, close_radius: float = 1.0,
              rng=RANGE):
    """points (B, S, N, C) fp32, counts (B, S), T (B, S, 4, 4) fp64, lag (B, S) fp32 ->
    (out (B, max_points, C + 1) fp32, count (B,) int32, sweep_count (B, S) int32)."""
    B, S, N, C = points.shape
    out = np.zeros((B, max_points, C + 1), dtype=np.float32)
    count, sweep_count = np.zeros(B, dtype=np.int32), np.zeros((B, S), dtype=np.int32)
    for b in range(B):
        rows = []
        for s in range(S):
            n = min(max(int(counts[b, s]), 0), N)
            p = points[b, s, :n]
            keep, q = keep_ref(T[b, s], p, close_radius, rng)
            r = np.empty((int(keep.sum()), C + 1), dtype=np.float32)
            r[:, :3], r[:, 3:C], r[:, C] = q[keep], p[keep, 3:], np.float32(lag[b, s])
            rows.append(r)
            sweep_count[b, s] = len(r)
        allrows = np.concatenate(rows) if rows else np.zeros((0, C + 1), dtype=np.float32)
        count[b] = len(allrows)
        k = min(len(allrows), max_points)
        out[b, :k].view(np.uint32)[:] = allrows[:k].view(np.uint32)
    return out, count, sweep_count


# ---- restatement: pose chain -------------------------------------------------------------------------------------------------------

def _inv_ref(M):
    """Rigid inverse (R^T, -(R^T t)) of the top 3 x 4; bottom row 0 0 0 1."""
    o = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            o[i, j] = M[j, i]
        o[i, 3] = -((M[0, i] * M[0, 3] + M[1, i] * M[1, 3]) + M[2, i] * M[2, 3])
    o[3, 3] = 1.0
    return o


def _mul_ref(X, Y):
    """Rows 0-2 of X . Y with both bottom rows taken as 0 0 0 1, element = (((a0 b0 + a1 b1) + a2 b2) + a3 b3)."""
    y = Y.copy()
    y[3] = (0.0, 0.0, 0.0, 1.0)
    o = np.zeros((4, 4))
    for i in range(3):
        for j in range(4):
            o[i, j] = ((X[i, 0] * y[0, j] + X[i, 1] * y[1, j]) + X[i, 2] * y[2, j]) + X[i, 3] * y[3, j]
    o[3, 3] = 1.0
    return o


def pose_chain_ref(key_l2e, key_e2g, sweep_l2e, sweep_e2g) -> np.ndarray:
    """(B, 4, 4), (B, 4, 4), (B, S, 4, 4), (B, S, 4, 4) fp64 -> T (B, S, 4, 4) = inv(L_k) . inv(E_k) . E_s . L_s, right to left; a sweep
    whose two poses equal the key's element for element (the key sweep itself) gets the exact identity."""
    B, S = sweep_l2e.shape[:2]
    T = np.zeros((B, S, 4, 4))
    for b in range(B):
        for s in range(S):
            if np.array_equal(sweep_l2e[b, s, :3], key_l2e[b, :3]) and np.array_equal(sweep_e2g[b, s, :3], key_e2g[b, :3]):
                T[b, s] = np.eye(4)
            else:
                T[b, s] = _mul_ref(_inv_ref(key_l2e[b]), _mul_ref(_inv_ref(key_e2g[b]), _mul_ref(sweep_e2g[b, s], sweep_l2e[b, s])))
    return T


# ---- plain formulation -------------------------------------------------------------------------------------------------------------

def merge_plain(points, counts, T, lag, close_radius: float = 1.0, rng=RANGE):
    """Per frame: (positions (k, 3) float64 before any rounding, source (k, 2) = (sweep, row) of every survivor, in output order)."""
    B, S, N, C = points.shape
    lo, hi = np.array(rng[:3]), np.array(rng[3:])
    frames = []
    for b in range(B):
        pos, src = [], []
        for s in range(S):
            n = int(np.clip(counts[b, s], 0, N))
            p = points[b, s, :n, :3].astype(np.float64)
            q = p @ T[b, s, :3, :3].T + T[b, s, :3, 3]
            mask = ((q > lo) & (q < hi)).all(1)
            if close_radius > 0:
                mask &= ~((np.abs(p[:, 0]) < close_radius) & (np.abs(p[:, 1]) < close_radius))
            pos.append(q[mask])
            src.append(np.stack([np.full(int(mask.sum()), s), np.nonzero(mask)[0]], 1))
        frames.append((np.concatenate(pos), np.concatenate(src)))
    return frames


def pose_chain_plain(key_l2e, key_e2g, sweep_l2e, sweep_e2g) -> np.ndarray:
    return np.linalg.inv(key_l2e)[:, None] @ np.linalg.inv(key_e2g)[:, None] @ sweep_e2g @ sweep_l2e


# ---- scenes ------------------------------------------------------------------------------------------------------------------------

def rot(yaw: float, pitch: float = 0.0, roll: float = 0.0) -> np.ndarray:
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def rigid(yaw, pitch, roll, t) -> np.ndarray:
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = rot(yaw, pitch, roll), t
    return M


def sweep_matrices(B: int, S: int, seed: int = 11) -> np.ndarray:
    """(B, S, 4, 4) fp64 non-trivial rigid transforms: sweep 0 a small motion too (the merge does not special-case it), older sweeps
    further away, as an ego vehicle at some metres per sweep would give."""
    rs = np.random.RandomState(seed)
    T = np.zeros((B, S, 4, 4))
    for b in range(B):
        for s in range(S):
            T[b, s] = rigid(rs.uniform(-0.05, 0.05) * (s + 1), rs.uniform(-0.01, 0.01), rs.uniform(-0.01, 0.01),
                            (rs.uniform(-0.6, 0.6) * (s + 1), rs.uniform(-0.2, 0.2) * (s + 1), rs.uniform(-0.05, 0.05)))
    return T


def lags(B: int, S: int) -> np.ndarray:
    """(B, S) fp32: 0.05 s per sweep plus a per-frame jitter, distinct for every (frame, sweep)."""
    return (0.05 * np.arange(S)[None, :] + 0.001 * np.arange(B)[:, None] + 0.0003).astype(np.float32)


def random_points(rs, shape, C: int) -> np.ndarray:
    """fp32 (*shape, C): x, y in +-60 m and z in -6 .. 4 m (some out of range), the other channels in 0 .. 255."""
    cols = [rs.uniform(-60, 60, shape), rs.uniform(-60, 60, shape), rs.uniform(-6, 4, shape)] + [rs.uniform(0, 255, shape) for _ in range(C - 3)]
    return np.stack(cols, -1).astype(np.float32)


def boundary_distance(T: np.ndarray, pts: np.ndarray, close_radius: float, rng=RANGE) -> np.ndarray:
    """Smallest distance (m) of each point to a decision boundary: a range face after the transform, the close square before it."""
    q = pts[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d = np.minimum(np.abs(q - np.array(rng[:3])), np.abs(q - np.array(rng[3:]))).min(1)
    if close_radius > 0:
        a = np.abs(pts[:, :2].astype(np.float64))
        d = np.minimum(d, np.abs(a - close_radius).min(1))
    return d


def keep_margin(points: np.ndarray, T: np.ndarray, close_radius: float) -> np.ndarray:
    """A point within 2 * MARGIN of a decision boundary is replaced by INTERIOR (in place, every row, valid or not), so that the
    margin condition (MARGIN) holds by construction and no test has to exclude anything."""
    B, S = points.shape[:2]
    for b in range(B):
        for s in range(S):
            near = boundary_distance(T[b, s], points[b, s], close_radius) < 2 * MARGIN
            points[b, s, near, :3] = INTERIOR
    return points


def surviving_points(rs, n: int, C: int, T: np.ndarray, close_radius: float) -> np.ndarray:
    """(n, C) fp32 rows that all survive under T: drawn well inside the range and outside the close square."""
    p = random_points(rs, (n,), C)
    p[:, 0] = rs.uniform(2.0, 40.0, n) * rs.choice([-1.0, 1.0], n)
    p[:, 1] = rs.uniform(-40.0, 40.0, n)
    p[:, 2] = rs.uniform(-3.0, 1.0, n)
    assert keep_ref(T, p, close_radius)[0].all()
    return p


EDGE = dict(B=4, S=3, N=1100, C=4, max_points=1500, close_radius=1.0)
EDGE_COUNTS = np.array([[1100, 1100, 1100], [0, 1, 1024], [0, 0, 0], [750, 750, 300]], dtype=np.int32)


def edge_scene():
    """The edge batch of test 1: (points (4, 3, 1100, 4), counts (4, 3), T, lag).  Frame 0: three full sweeps of mostly surviving rows,
    the cut inside sweep 1.  Frame 1: an empty key sweep, one surviving point, one full tile.  Frame 2: nothing.  Frame 3: 750 + 750 rows
    that all survive, so the cut falls exactly on the boundary to sweep 2.  Rows past the counts hold in-range garbage."""
    B, S, N, C, r = EDGE["B"], EDGE["S"], EDGE["N"], EDGE["C"], EDGE["close_radius"]
    rs = np.random.RandomState(77)
    T, lag = sweep_matrices(B, S), lags(B, S)
    pts = random_points(rs, (B, S, N), C)
    pts[0, :, :, :2] *= np.float32(0.7)                           # frame 0: |x|, |y| <= 42 m, mostly surviving
    pts[1, 1, 0, :3] = (3.0, 4.0, 0.5)                            # the single point of frame 1, sweep 1 survives
    for s in (0, 1):
        pts[3, s, :750] = surviving_points(rs, 750, C, T[3, s], r)
    for b in range(B):                                            # in-range garbage past the counts
        for s in range(S):
            n = int(EDGE_COUNTS[b, s])
            pts[b, s, n:, :3] = np.array([5.0, 6.0, 0.25], dtype=np.float32) + rs.uniform(-1, 1, (N - n, 3)).astype(np.float32)
    return keep_margin(pts, T, r), EDGE_COUNTS.copy(), T, lag


def small_scene(B: int, S: int, N: int, C: int, seed: int, close_radius: float = 1.0, counts=None):
    """A generic scene with the margin kept: (points, counts, T, lag); counts default to random values in 0 .. N."""
    rs = np.random.RandomState(seed)
    T, lag = sweep_matrices(B, S, seed), lags(B, S)
    pts = keep_margin(random_points(rs, (B, S, N), C), T, close_radius)
    if counts is None:
        counts = rs.randint(0, N + 1, (B, S))
    return pts, np.asarray(counts, dtype=np.int32).reshape(B, S), T, lag


def special_rows(C: int = 4):
    """Test 3: (points (1, 1, 7, C), names) under the exactly-identity transform with close_radius 1: what each row is."""
    p = np.zeros((7, C), dtype=np.float32)
    p[:, 3:] = np.arange(7 * (C - 3), dtype=np.float32).reshape(7, C - 3) + 1
    p[0, :3] = (np.nan, 2.0, 0.0)                                 # NaN x: dropped
    p[1, :3] = (3.0, 2.0, np.inf)                                 # +inf z: dropped
    p[2, :3] = (np.float32(RANGE[3]), 2.0, 0.0)                   # exactly on the x1 face: dropped (strict)
    p[3, :3] = (1.0, 0.25, 0.0)                                   # |x| == r exactly: kept
    p[4, :3] = (0.5, -1.0, 0.0)                                   # |x| < r, |y| >= r: kept
    p[5, :3] = (-0.5, 0.99, 0.0)                                  # inside the close square: dropped
    p[6, :3] = (-12.625, 7.3, -0.75)                              # ordinary: keeps its bits (1 * v plus zeros is exact for v != 0)
    names = ["nan x", "+inf z", "on a range face", "|x| == r", "|x| < r, |y| >= r", "inside the close square", "ordinary"]
    return p[None, None].copy(), names, np.array([False, False, False, True, True, False, True])


def pose_scene(B: int = 3, S: int = 4, seed: int = 21):
    """Calibration with global translations near (1000, 600, 0) m and yaw, pitch and roll: (key_l2e (B, 4, 4), key_e2g (B, 4, 4),
    sweep_l2e (B, S, 4, 4), sweep_e2g (B, S, 4, 4)) fp64.  Sweep 0 is the key sweep itself (its poses are the key's)."""
    rs = np.random.RandomState(seed)
    kl, ke = np.zeros((B, 4, 4)), np.zeros((B, 4, 4))
    sl, se = np.zeros((B, S, 4, 4)), np.zeros((B, S, 4, 4))
    for b in range(B):
        lidar = rigid(rs.uniform(-0.02, 0.02) - np.pi / 2, rs.uniform(-0.01, 0.01), rs.uniform(-0.01, 0.01), (0.94, 0.0, 1.84))
        yaw, pos = rs.uniform(-np.pi, np.pi), np.array([1000.0, 600.0, 0.0]) + rs.uniform(-50, 50, 3) * (1, 1, 0.02)
        kl[b], ke[b] = lidar, rigid(yaw, rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), pos)
        for s in range(S):
            if s == 0:
                sl[b, s], se[b, s] = kl[b], ke[b]
                continue
            back = 0.5 * s * np.array([np.cos(yaw), np.sin(yaw), 0.0])            # 10 m/s at 20 Hz, driven backwards in time
            sl[b, s] = lidar
            se[b, s] = rigid(yaw - 0.01 * s + rs.uniform(-0.002, 0.002), rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03),
                             pos - back + rs.uniform(-0.02, 0.02, 3))
    return kl, ke, sl, se
