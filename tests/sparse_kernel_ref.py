"""TEST INFRASTRUCTURE -- per-kernel references of the sparse-voxel LiDAR encoder (csrc/sparse_index.hip, sparse_conv.hip,
sparse_rows.hip; DESIGN.md 3.2b3, "kernel-level pins"), and the cases the kernel tests run.  CPU only, plain torch / numpy, no
project kernel: everything works on the flat buffers the `_lib.sparse_*` wrappers take, in fp64 unless integers are exact.
tests/test_sparse_kernels_host.py shows on the CPU that these references are the dense conv3d semantics of tests/sparse_ref.py
and that every case has the property it is built for; tests/test_gpu_sparse_kernels.py runs the kernels against them.

Rows and slots: a level is `cap` row slots per frame, row r = b * cap + v is active iff v < count[b].  The integer references
return whole buffers: slots the kernel must not write hold INT_SENTINEL, which is what the GPU tests prefill them with."""
import numpy as np
import torch
import torch.nn.functional as F

INT_SENTINEL = -12345         # prefill of integer outputs
FLOAT_SENTINEL = -7.0         # prefill of float outputs (where the case does not ask for NaN)
WIDTHS = (32, 64, 96, 128)
ROW_TILE = 128                # sparse_conv: output rows per workgroup
WGRAD_STEP = 32               # sparse_wgrad: rows per K step
WGRAD_CHUNKS = 32             # sparse_wgrad: row chunks = partial sums per tap
BN_WORKGROUPS = 256           # sp_bn_sums: workgroups of the reduction


def active_mask(count, B, cap):
    """(B * cap,) bool: slot v of frame b is active iff v < count[b]."""
    count = torch.as_tensor(count).long().view(B, 1)
    assert int(count.max()) <= cap and int(count.min()) >= 0              # count > cap is not a reachable state
    return (torch.arange(cap).view(1, cap) < count).reshape(-1)


# ---- structure (integers, exact) -------------------------------------------------------------------------------------------

def fill_index_ref(coords, count, B, cap, dims):
    """coords [B * cap][3] int64 (z, y, x) -> index volume [B][D][H][W] int32 (row or -1), cell [B * cap] int32 (linear cell of an
    active row, -1 for an active row outside the grid, INT_SENTINEL in inactive slots)."""
    D, H, W = dims
    coords = torch.as_tensor(coords).view(B * cap, 3).long()
    act = active_mask(count, B, cap)
    index = torch.full((B, D, H, W), -1, dtype=torch.int32)
    cell = torch.full((B * cap,), INT_SENTINEL, dtype=torch.int32)
    for r in act.nonzero().flatten().tolist():
        z, y, x = coords[r].tolist()
        if 0 <= z < D and 0 <= y < H and 0 <= x < W:
            index[r // cap, z, y, x] = r
            cell[r] = (z * H + y) * W + x
        else:
            cell[r] = -1
    return index, cell


def down_ref(index_in, B, dims, cap_out):
    """3x3x3 / stride 2 / pad 1: active outputs are max_pool3d(occ, 3, 2, 1) > 0, rows in raster (z, y, x) order, the count
    clamped to cap_out, cells past the cap get index -1.  -> index_out [B][D/2][H/2][W/2], cell_out [B * cap_out], count_out [B]."""
    D, H, W = dims
    occ = (torch.as_tensor(index_in).view(B, 1, D, H, W) >= 0).double()
    act = F.max_pool3d(occ, 3, 2, 1)[:, 0] > 0
    index_out = torch.full(act.shape, -1, dtype=torch.int32)
    cell_out = torch.full((B * cap_out,), INT_SENTINEL, dtype=torch.int32)
    count_out = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        cells = act[b].flatten().nonzero().flatten()
        n = min(int(cells.numel()), cap_out)
        count_out[b] = n
        rows = b * cap_out + torch.arange(n)
        index_out[b].view(-1)[cells[:n]] = rows.int()
        cell_out[rows] = cells[:n].int()
    return index_out, cell_out, count_out


def table_ref(index, cell, count, B, cap, in_dims, row_dims, stride, transposed):
    """Neighbour table [B * cap][27] int32 of the rows whose cells live in `row_dims`, looking into the volume `index` of
    `in_dims`; tap k = (kz * 3 + ky) * 3 + kx.  Forward: in = out * stride - 1 + k.  Transposed: out = (in + 1 - k) / stride when
    in + 1 - k >= 0 and the division is exact.  -1 = absent; a row with cell == -1 is all -1; inactive slots INT_SENTINEL."""
    (Di, Hi, Wi), (Dr, Hr, Wr) = in_dims, row_dims
    index = torch.as_tensor(index).view(B, Di, Hi, Wi)
    cell = torch.as_tensor(cell).view(-1)
    act = active_mask(count, B, cap)
    table = torch.full((B * cap, 27), INT_SENTINEL, dtype=torch.int32)

    def tap(c, k, n):
        if not transposed:
            t = c * stride - 1 + k
        else:
            t = c + 1 - k
            if t < 0 or t % stride:
                return None
            t //= stride
        return t if 0 <= t < n else None

    for r in act.nonzero().flatten().tolist():
        table[r] = -1
        c = int(cell[r])
        if c < 0:
            continue
        z, y, x = c // (Wr * Hr), (c // Wr) % Hr, c % Wr
        for k in range(27):
            zi, yi, xi = tap(z, k // 9, Di), tap(y, (k // 3) % 3, Hi), tap(x, k % 3, Wi)
            if zi is not None and yi is not None and xi is not None:
                table[r, k] = index[r // cap, zi, yi, xi]
    return table


# ---- mean VFE (fp32, bit-exact) --------------------------------------------------------------------------------------------

def vfe_mean_ref(feats, npts, nvox, B, Nv, P, C, Cpad, fill=float("nan")):
    """rows [B * Nv][Cpad] fp32: the mean of a voxel's first clamp(npts, 0, P) points, the sum taken in point order (one IEEE fp32
    addition per point: the same bits as the kernel's loop), one division; channels C .. Cpad - 1 zero; inactive slots `fill`."""
    f = np.asarray(torch.as_tensor(feats).view(B * Nv, P, C).numpy(), dtype=np.float32)
    n = np.clip(torch.as_tensor(npts).view(-1).numpy().astype(np.int64), 0, P)
    act = active_mask(nvox, B, Nv).numpy()
    s = np.zeros((B * Nv, C), dtype=np.float32)
    for p in range(P):
        s = np.where((p < n)[:, None], (s + f[:, p, :]).astype(np.float32), s)
    mean = np.where((n > 0)[:, None], s / np.maximum(n, 1).astype(np.float32)[:, None], np.float32(0)).astype(np.float32)
    rows = np.full((B * Nv, Cpad), fill, dtype=np.float32)
    rows[act] = 0
    rows[act, :C] = mean[act]
    return torch.from_numpy(rows)


# ---- the gather-GEMM ---------------------------------------------------------------------------------------------------------

def gather_gemm(x, table, active, w_packed, Cin, Cout, dtype=torch.float64):
    """y[r] = sum_k x[table[r][k]] @ w[k] over the active rows r (0 in inactive slots), absent entries (-1) contributing zero;
    w_packed is the kernel's [27][Cin][Cout].  index_select / matmul / index_add only, so autograd gives dx and dw; rows of x that
    no active entry names are never touched (they may hold NaN).  The fp64 instance is the reference."""
    table = torch.as_tensor(table).view(-1, 27).long()
    w = w_packed.view(27, Cin, Cout).to(dtype)
    x = x.view(-1, Cin).to(dtype)
    y = torch.zeros(table.shape[0], Cout, dtype=dtype)
    for k in range(27):
        rows = (active & (table[:, k] >= 0)).nonzero().flatten()
        if rows.numel():
            y = y.index_add(0, rows, x.index_select(0, table[rows, k]) @ w[k])
    return y


def _gathered(x, table, active, Cin):
    """fp32 numpy [R][27][Cin]: x[table[r][k]], zero where the entry is absent or the row inactive."""
    table = torch.as_tensor(table).view(-1, 27).long()
    have = active[:, None] & (table >= 0)
    xg = torch.as_tensor(x).view(-1, Cin).float()[table.clamp_min(0)]
    return torch.where(have[..., None], xg, torch.zeros(())).numpy()


def gather_gemm_seq32(x, table, active, w_packed, Cin, Cout):
    """The yardstick of the forward and the data gradient: the same sum in fp32, accumulated term by term in K order (tap, then
    channel) with separately rounded np.float32 products and additions.  Rows and output channels vectorised; K <= 27 * 128."""
    w = w_packed.view(27, Cin, Cout).float().numpy()
    act = active.nonzero().flatten()
    xg = _gathered(x, table, active, Cin)[act.numpy()]
    acc = np.zeros((xg.shape[0], Cout), dtype=np.float32)
    for k in range(27):
        if not xg[:, k].any():
            continue                                                          # (every term is an exact zero)
        for c in range(Cin):
            acc += xg[:, k, c, None] * w[k, c][None, :]
    y = torch.zeros(active.numel(), Cout)
    y[act] = torch.from_numpy(acc)
    return y


def wgrad_seq32(x, dy, table, active, Cin, Cout):
    """The yardstick of the weight gradient: dw[k] = sum over rows of x[table[r][k]]^T dy[r] in fp32, row after row in row order.
    -> [27][Cin][Cout] (the packed layout)."""
    act = active.nonzero().flatten().numpy()
    xg = _gathered(x, table, active, Cin)[act]
    g = torch.as_tensor(dy).view(-1, Cout).float().numpy()[act]
    acc = np.zeros((27, Cin, Cout), dtype=np.float32)
    for r in range(xg.shape[0]):
        acc += xg[r][:, :, None] * g[r][None, None, :]
    return torch.from_numpy(acc)


def dw_torch_layout(dw_packed, Cin, Cout, cin_real):
    """[27][Cin][Cout] -> torch's Conv3d layout [Cout][cin_real][27], flat."""
    return dw_packed.view(27, Cin, Cout)[:, :cin_real].permute(2, 1, 0).contiguous().view(-1)


def epilogue(y, scale, shift, relu):
    """acc * scale + shift, ReLU, in y's dtype (fp64: the reference; fp32: the yardstick)."""
    if scale is not None:
        y = y * scale.to(y.dtype)
    if shift is not None:
        y = y + shift.to(y.dtype)
    return y.clamp_min(0) if relu else y


# ---- BatchNorm over the active rows ----------------------------------------------------------------------------------------

def bn_rows_ref(y, active, gamma, beta, eps, momentum, rmean, rvar, nbt, frozen=False):
    """BatchNorm1d + ReLU over the active rows in fp64 with autograd: two-pass variance; running buffers as nn.BatchNorm1d moves
    them (momentum=None: cumulative average with num_batches_tracked; untouched when N < 2 or frozen).  frozen: the statistics are
    the running buffers.  -> dict(rows, pre, a, mean, var, invstd, rmean, rvar, nbt, N); `rows` is the leaf whose .grad is dy."""
    C = y.shape[-1]
    rows = y.view(-1, C)[active].double().clone().requires_grad_()
    N = rows.shape[0]
    rm, rv = rmean.double().clone(), rvar.double().clone()
    nbt = int(nbt)
    if frozen:
        mean, var = rm, rv
    else:
        mean = rows.mean(0)
        var = ((rows - mean) ** 2).mean(0)
        if N > 1:
            mo = 1.0 / (nbt + 1) if momentum is None else float(momentum)
            rm = (1 - mo) * rm + mo * mean.detach()
            rv = (1 - mo) * rv + mo * var.detach() * N / (N - 1)
            nbt += 1
    invstd = 1.0 / torch.sqrt(var + eps)
    pre = (rows - mean) * invstd
    if gamma is not None:
        pre = pre * gamma.double()
    if beta is not None:
        pre = pre + beta.double()
    return dict(rows=rows, pre=pre, a=F.relu(pre), mean=mean.detach(), var=var.detach(), invstd=invstd.detach(), rmean=rm, rvar=rv,
                nbt=nbt, N=N)


def bn_invstd_one_pass_f32(rows, eps):
    """What an fp32 accumulation of the kernel's one-pass formula (sum y, sum y^2 in row order) would give: the large-mean case
    shows that it cannot meet the bound the fp64 partials meet."""
    r = rows.float().numpy()
    s1 = np.zeros(r.shape[1], dtype=np.float32)
    s2 = np.zeros(r.shape[1], dtype=np.float32)
    for i in range(r.shape[0]):
        s1 += r[i]
        s2 += r[i] * r[i]
    n = np.float32(r.shape[0])
    m = s1 / n
    var = np.maximum(s2 / n - m * m, np.float32(0))
    return torch.from_numpy(np.float32(1) / np.sqrt(var + np.float32(eps)))


def ulps(a, b):
    """Largest distance, in fp32 units in the last place, between a (fp32) and b rounded to fp32."""
    def key(t):
        i = t.float().contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a.cpu().flatten()) - key(torch.as_tensor(b).flatten())).abs().max())


# ---- canvas ------------------------------------------------------------------------------------------------------------------

def canvas_ref(rows, cell, count, B, cap, dims, C):
    """canvas[b][y][x][z * C + c] = rows[row][c] at the row's cell (z, y, x); everything else exactly 0."""
    D, H, W = dims
    rows, cell = rows.view(B * cap, C), torch.as_tensor(cell).view(-1).long()
    canvas = torch.zeros(B, H * W, D * C, dtype=rows.dtype)
    for r in active_mask(count, B, cap).nonzero().flatten().tolist():
        cl = int(cell[r])
        if 0 <= cl < D * H * W:
            z, yx = cl // (H * W), cl % (H * W)
            canvas[r // cap, yx, z * C:(z + 1) * C] = rows[r]
    return canvas.view(B, H, W, D * C)


def canvas_bwd_ref(dcanvas, cell, count, B, cap, dims, C, fill=FLOAT_SENTINEL):
    """The gather that is canvas_ref's backward: drows[row] = dcanvas at the row's cell, 0 for a row without a cell; inactive
    slots `fill`."""
    D, H, W = dims
    dc, cell = dcanvas.view(B, H * W, D * C), torch.as_tensor(cell).view(-1).long()
    drows = torch.full((B * cap, C), fill, dtype=dcanvas.dtype)
    for r in active_mask(count, B, cap).nonzero().flatten().tolist():
        cl = int(cell[r])
        drows[r] = 0
        if 0 <= cl < D * H * W:
            z, yx = cl // (H * W), cl % (H * W)
            drows[r] = dc[r // cap, yx, z * C:(z + 1) * C]
    return drows


# ---- cases ---------------------------------------------------------------------------------------------------------------------
# Built once per key, shared by the host and the GPU file, never modified (callers clone what they change).

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _gen(*seed):
    v = 0
    for s in seed:
        v = (v * 1000003 + int(s) + 1) % (1 << 31)
    return torch.Generator().manual_seed(v)


# sparse_conv / sparse_wgrad row layouts: name -> (B, cap, counts)
CONV_LAYOUTS = {
    "straddle": (3, 200, [200, 0, 129]),       # tile 1 straddles frames 0 / 1, tile 3 frames 1 / 2, frame 1 empty, frame 2 ends one past a tile edge
    "four-frames": (5, 40, [40, 3, 0, 40, 17]),  # tile 0 spans frames 0 .. 3
    "one-127": (1, 256, [127]), "one-128": (1, 256, [128]), "one-129": (1, 256, [129]),
}
WGRAD_LAYOUTS = {
    "straddle": CONV_LAYOUTS["straddle"],      # 600 slots = 19 row steps: 13 of the 32 chunks own no step
    "three-rounds": (2, 1100, [1100, 130]),    # 2200 slots = 69 steps: up to three rounds of the chunk loop, cap % 32 != 0
    "one-ragged": (1, 31, [31]),               # a single ragged step
}
ROWS_IN = 333                                  # x rows of the synthetic tables: a space of its own, not a multiple of anything
NO_NEIGHBOUR = (5, 9)                          # active rows whose table row is all -1
TRIPLE_ROW, TRIPLE_TAPS = 17, (1, 4, 22)       # one row with the same input row under three taps
X_POOL = 300                                   # rows of x the active table entries draw from; the rest are only named by inactive slots


def synth_table(layout, wgrad=False):
    """A non-geometric table for a row layout -> dict(B, cap, count, active, table [B * cap][27] int32, named (ROWS_IN,) bool).
    Active entries are drawn from X_POOL rows of x with about half absent; tap 13 is absent in every row of tile 0 (wgrad: in every
    row); tap 0 is present in exactly one row of tile 1 (`single`, if tile 1 has an active row); rows NO_NEIGHBOUR are all -1;
    TRIPLE_ROW has one input row under TRIPLE_TAPS.  Inactive slots hold valid row numbers of x that no active entry names:
    the tests poison those rows with NaN."""
    def make():
        B, cap, counts = (WGRAD_LAYOUTS if wgrad else CONV_LAYOUTS)[layout]
        g = _gen(11, len(layout), B, cap, int(wgrad))
        R = B * cap
        act = active_mask(counts, B, cap)
        pool = torch.randperm(ROWS_IN, generator=g)
        pool, rest = pool[:X_POOL], pool[X_POOL:]
        tab = pool[torch.randint(0, X_POOL, (R, 27), generator=g)]
        tab[torch.rand(R, 27, generator=g) < 0.5] = -1
        tab[:R if wgrad else ROW_TILE, 13] = -1
        single = None
        t1 = act[ROW_TILE:2 * ROW_TILE].nonzero().flatten() + ROW_TILE
        if t1.numel():
            single = int(t1[t1.numel() // 2])
            tab[ROW_TILE:2 * ROW_TILE, 0] = -1
            tab[single, 0] = pool[7]
        for r in NO_NEIGHBOUR:
            tab[r] = -1
        tab[TRIPLE_ROW, list(TRIPLE_TAPS)] = pool[3]
        tab[~act] = rest[torch.randint(0, rest.numel(), (int((~act).sum()), 27), generator=g)]
        named = torch.zeros(ROWS_IN, dtype=torch.bool)
        e = tab[act]
        named[e[e >= 0]] = True
        return dict(B=B, cap=cap, count=torch.tensor(counts, dtype=torch.int32), active=act, table=tab.int().contiguous(),
                    named=named, single=single)
    return _cached(("table", layout, wgrad), make)


def conv_inputs(layout, Cin, Cout, wgrad=False):
    """x [ROWS_IN][Cin] ~ N(0, 1) with NaN in the rows no active entry names, w [27][Cin][Cout] ~ 0.1 N(0, 1) (flat), scale in
    (0.5, 1.5), shift ~ 0.5 N(0, 1), dy [B * cap][Cout] ~ N(0, 1) with NaN in inactive slots."""
    def make():
        t = synth_table(layout, wgrad)
        g = _gen(13, len(layout), Cin, Cout, int(wgrad))
        x = torch.randn(ROWS_IN, Cin, generator=g)
        x[~t["named"]] = float("nan")
        dy = torch.randn(t["B"] * t["cap"], Cout, generator=g)
        dy[~t["active"]] = float("nan")
        return dict(x=x, w=(0.1 * torch.randn(27 * Cin * Cout, generator=g)), scale=0.5 + torch.rand(Cout, generator=g),
                    shift=0.5 * torch.randn(Cout, generator=g), dy=dy)
    return _cached(("conv_in", layout, Cin, Cout, wgrad), make)


def slot_permutation(t):
    """A permutation of the active slots within each frame -> (perm (B * cap,) with perm[r] = the slot row r moves to, table of the
    permuted layout).  Inactive slots stay where they are."""
    g = _gen(17, t["B"], t["cap"])
    perm = torch.arange(t["B"] * t["cap"])
    for b, n in enumerate(t["count"].tolist()):
        perm[b * t["cap"]:b * t["cap"] + n] = b * t["cap"] + torch.randperm(n, generator=g)
    tab = t["table"].clone()
    tab[perm] = t["table"]
    return perm, tab


# the device-built structure of the table and data-gradient tests: level 0 (4, 32, 28), three frames, level 1 (2, 16, 14)
STRUCT = dict(B=3, dims0=(4, 32, 28), dims1=(2, 16, 14), cap0=100, cap1=180, spare=(1, 1, 1), random=60)


def structure_coords():
    """-> (coords [B * cap0][3] int64, count [B] int32).  Frame 0 is tests/sparse_scenes.structured_voxels (isolated voxel, solid
    4x4x4 block, corners, faces); frame 1 is random cells plus one active row outside the grid (z = D: its cell is -1); frame 2 is
    empty.  Inactive slots hold the in-grid cell `spare`, which no frame activates: a kernel that processed one would show in the
    index volume."""
    def make():
        from tests import sparse_scenes as S
        D, H, W = STRUCT["dims0"]
        B, cap = STRUCT["B"], STRUCT["cap0"]
        f0 = [v for part in S.structured_voxels(D, H, W) for v in part]
        g = _gen(19)
        sp = (STRUCT["spare"][0] * H + STRUCT["spare"][1]) * W + STRUCT["spare"][2]
        cells = [c for c in torch.randperm(D * H * W, generator=g).tolist() if c != sp][:STRUCT["random"]]
        f1 = [(c // (H * W), (c // W) % H, c % W) for c in cells]
        f1.insert(20, (D, 3, 3))
        coords = torch.tensor(STRUCT["spare"], dtype=torch.int64).repeat(B * cap, 1)
        coords[:len(f0)] = torch.tensor(f0)
        coords[cap:cap + len(f1)] = torch.tensor(f1)
        return coords.contiguous(), torch.tensor([len(f0), len(f1), 0], dtype=torch.int32)
    return _cached("structure", make)


def structure_ref():
    """The whole structure from the references: index0 / cell0 / count0, index1 / cell1 / count1 and the four tables
    (stride, transposed) -> table."""
    def make():
        s = STRUCT
        coords, count0 = structure_coords()
        index0, cell0 = fill_index_ref(coords, count0, s["B"], s["cap0"], s["dims0"])
        index1, cell1, count1 = down_ref(index0, s["B"], s["dims0"], s["cap1"])
        tabs = {
            (1, False): table_ref(index0, cell0, count0, s["B"], s["cap0"], s["dims0"], s["dims0"], 1, False),
            (2, False): table_ref(index0, cell1, count1, s["B"], s["cap1"], s["dims0"], s["dims1"], 2, False),
            (2, True): table_ref(index1, cell0, count0, s["B"], s["cap0"], s["dims1"], s["dims0"], 2, True),
            (1, True): table_ref(index0, cell0, count0, s["B"], s["cap0"], s["dims0"], s["dims0"], 1, True),
        }
        return dict(index0=index0, cell0=cell0, count0=count0, index1=index1, cell1=cell1, count1=count1, tables=tabs)
    return _cached("structure_ref", make)


def inverse_relation(t_f, act_o, t_t, act_i):
    """T_f[o][k] == i  iff  T_t[i][k] == o, over all active o, i and all k: the two sets of (o, k, i) triples are equal."""
    def triples(t, act, swap):
        t = torch.as_tensor(t).view(-1, 27).long()
        r, k = (act[:, None] & (t >= 0)).nonzero(as_tuple=True)
        e = t[r, k]
        return set(zip(*(x.tolist() for x in ((e, k, r) if swap else (r, k, e)))))
    return triples(t_f, act_o, False) == triples(t_t, act_i, True)


# sparse_down: input dims -> why
DOWN_DIMS = {
    (2, 6, 10): "Do = 1, 15 output cells",
    (4, 8, 12): "48 output cells, far below one scan block",
    (8, 8, 24): "192 output cells, below one scan block",
    (16, 16, 32): "exactly 1024 output cells",
    (8, 36, 50): "1800 output cells: a ragged second chunk in scan_counts",
}


def down_case(dims, cap_binds=False):
    """index_in [4][D][H][W] int32 for sparse_down: frame 0 random (about 10 %), frame 1 empty, frame 2 full, frame 3 a single voxel
    at the far corner; rows numbered b * cells + order of appearance (any non-negative value marks a cell).  -> (index_in, cap_out):
    cap_out is the number of output cells (nothing truncated), or with cap_binds half the active outputs of the random frame."""
    def make():
        D, H, W = dims
        cells = D * H * W
        g = _gen(23, D, H, W)
        occ = torch.zeros(4, cells, dtype=torch.bool)
        occ[0] = torch.rand(cells, generator=g) < 0.1
        occ[2] = True
        occ[3, cells - 1] = True
        index = torch.full((4, cells), -1, dtype=torch.int32)
        for b in range(4):
            c = occ[b].nonzero().flatten()
            index[b, c] = (b * cells + torch.arange(c.numel())).int()
        index = index.view(4, D, H, W)
        cells_o = cells // 8
        if cap_binds:
            n0 = int((F.max_pool3d((index[:1, None] >= 0).double(), 3, 2, 1) > 0).sum())
            return index, max(1, n0 // 2)
        return index, cells_o
    return _cached(("down", dims, cap_binds), make)


def bn_rows_case(layout, C, offset=0.0, seed=0):
    """y [B * cap][C] fp32 for the BatchNorm row kernels: `offset` + N(0, 1) scaled and shifted per channel, NaN in inactive slots;
    gamma in (0.5, 1.5), beta ~ 0.5 N(0, 1), running buffers, da ~ N(0, 1) with NaN in inactive slots.  The active rows are nudged
    until no pre-activation of relu(batchnorm(y)) lies within 1e-3 of 0, with batch statistics and with the running ones."""
    def make():
        B, cap, counts = BN_LAYOUTS[layout]
        g = _gen(29, len(layout), C, seed)
        act = active_mask(counts, B, cap)
        y = torch.randn(B * cap, C, generator=g)
        y = offset + y if offset else y * (0.5 + torch.rand(C, generator=g)) + 0.5 * torch.randn(C, generator=g)
        gamma, beta = 0.5 + torch.rand(C, generator=g), 0.5 * torch.randn(C, generator=g)
        rmean = y[act].mean(0) + 0.1 * torch.randn(C, generator=g)
        rvar = (y[act].var(0, unbiased=False) if int(act.sum()) > 1 else torch.ones(C)) * (0.8 + 0.4 * torch.rand(C, generator=g))
        da = torch.randn(B * cap, C, generator=g)
        if not offset and int(act.sum()) > 2:
            for _ in range(20):
                close = torch.zeros(int(act.sum()), C, dtype=torch.bool)
                for frozen in (False, True):
                    for ga, be in ((gamma, beta), (None, None)):
                        pre = bn_rows_ref(y, act, ga, be, 1e-5, 0.1, rmean, rvar, 0, frozen)["pre"].detach()
                        close |= pre.abs() < 2e-3
                if not close.any():
                    break
                rows = y[act]
                rows[close] += 0.05
                y[act] = rows
        y[~act] = float("nan")
        da[~act] = float("nan")
        return dict(B=B, cap=cap, count=torch.tensor(counts, dtype=torch.int32), active=act, y=y.contiguous(), gamma=gamma, beta=beta,
                    rmean=rmean.float(), rvar=rvar.float(), da=da)
    return _cached(("bn", layout, C, offset, seed), make)


BN_LAYOUTS = {
    "straddle": CONV_LAYOUTS["straddle"],
    "long": (1, 2100, [2077]),                 # more than BN_WORKGROUPS * (256 / 32) rows at C = 32: the per-workgroup stride loop repeats
    "one-row": (3, 200, [1, 0, 0]),
    "two-rows": (3, 200, [1, 0, 1]),
}


CANVAS = dict(B=2, cap=40, dims=(2, 5, 7), counts=[40, 9], lost=11)


def canvas_case(C):
    """rows [B * cap][C] ~ N(0, 1) with NaN in inactive slots, unique cells per frame, row `lost` with cell = -1; inactive slots
    carry valid cells (a kernel that wrote one would put a NaN into the canvas)."""
    def make():
        B, cap, (D, H, W) = CANVAS["B"], CANVAS["cap"], CANVAS["dims"]
        g = _gen(31, C)
        act = active_mask(CANVAS["counts"], B, cap)
        cell = torch.cat([torch.randperm(D * H * W, generator=g)[:cap] for _ in range(B)]).int()
        cell[CANVAS["lost"]] = -1
        rows = torch.randn(B * cap, C, generator=g)
        rows[~act] = float("nan")
        return dict(rows=rows, cell=cell, count=torch.tensor(CANVAS["counts"], dtype=torch.int32),
                    dcanvas=torch.randn(B, H, W, D * C, generator=g))
    return _cached(("canvas", C), make)


FILL = dict(B=3, cap=70, dims=(4, 8, 12), counts=[70, 0, 33], out_z=12, out_x=2 * 70 + 30)


def fill_index_case():
    """coords [B * cap][3] for sparse_fill_index: unique random cells per frame; active row `out_z` has z = D and active row `out_x`
    has x = -1 (their cell is -1, the index volume is untouched by them); inactive slots hold in-grid cells."""
    def make():
        B, cap, (D, H, W) = FILL["B"], FILL["cap"], FILL["dims"]
        g = _gen(37)
        c = torch.cat([torch.randperm(D * H * W, generator=g)[:cap] for _ in range(B)])
        coords = torch.stack([c // (H * W), (c // W) % H, c % W], 1)
        coords[FILL["out_z"], 0] = D
        coords[FILL["out_x"], 2] = -1
        return coords.contiguous(), torch.tensor(FILL["counts"], dtype=torch.int32)
    return _cached("fill", make)


VFE = dict(B=2, Nv=45, counts=[45, 7], Cpad=32, special={3: 0, 10: "P", 21: "P+3", 30: -1, 47: 0})


def vfe_case(C, P):
    """feats [B * Nv][P][C] ~ N(0, 1) (NaN in inactive slots), npts in 1 .. P with the rows of VFE['special'] set to 0, P, P + 3
    (clamped to P) and -1 (clamped to 0)."""
    def make():
        B, Nv = VFE["B"], VFE["Nv"]
        g = _gen(41, C, P)
        feats = torch.randn(B * Nv, P, C, generator=g)
        feats[~active_mask(VFE["counts"], B, Nv)] = float("nan")
        npts = torch.randint(1, P + 1, (B * Nv,), generator=g).int()
        for r, v in VFE["special"].items():
            npts[r] = {"P": P, "P+3": P + 3}.get(v, v)
        return feats.contiguous(), npts, torch.tensor(VFE["counts"], dtype=torch.int32)
    return _cached(("vfe", C, P), make)
