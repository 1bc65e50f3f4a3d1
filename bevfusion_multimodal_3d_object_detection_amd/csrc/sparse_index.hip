// Structure of the sparse-voxel LiDAR encoder (the opt-in `model.lidar_encoder.type: SparseVoxel` branch): which
// cells of each level are active, in which row their features live, and which rows a 3x3x3 filter tap reads.  No reference line
// (the reference has no working voxel path): the semantics are spconv's, pinned by tests/sparse_ref.py.
//   * a level is `cap` row slots per frame: row r = b * cap + v is active iff v < count[b] (count lives on the device; every grid
//     here is sized by capacity and threads past the count return: nothing is read back to size a launch);
//   * index volume [B][D][H][W] int32: the row of a cell, or -1.  Cells are unique per frame, so the scatter has no collisions;
//   * a strided level (3x3x3 / stride 2 / pad 1): output cell o is active iff some active input i has 2o-1 <= i <= 2o+1 on every
//     axis -- mark, a fixed-order scan over the cells (scan_counts.h), then rows in raster (z, y, x) order and the frame's count;
//   * neighbour table [rows][27] int32 (-1 = absent), tap k = (kz * 3 + ky) * 3 + kx: forward  in = out * stride - 1 + k;
//     transposed (the data gradient of a strided layer, rows = the layer's input rows)  out = (in + 1 - k) / stride when that divides.
#include "common.h"
#include "scan_counts.h"

namespace {

__device__ __forceinline__ bool row_active(const int32_t* __restrict__ count, int cap, long long row, int& b) {
  b = (int)(row / cap);
  const int v = (int)(row - (long long)b * cap);
  const int n = count[b];
  return v < (n < cap ? n : cap);
}

__global__ __launch_bounds__(256) void sp_fill_index(const long long* __restrict__ coords, const int32_t* __restrict__ count, int B, int cap,
                                                     int D, int H, int W, int32_t* __restrict__ index, int32_t* __restrict__ cell) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * cap) return;
  int b;
  if (!row_active(count, cap, i, b)) return;
  const long long z = coords[i * 3], y = coords[i * 3 + 1], x = coords[i * 3 + 2];
  if (z < 0 || z >= D || y < 0 || y >= H || x < 0 || x >= W) {       // (voxelize never emits one: such a row reads and writes nothing)
    cell[i] = -1;
    return;
  }
  const int c = (int)((z * H + y) * W + x);
  index[(long long)b * D * H * W + c] = (int32_t)i;
  cell[i] = c;
}

__global__ __launch_bounds__(256) void sp_down_mark(const int32_t* __restrict__ index_in, int B, int D, int H, int W,
                                                    int32_t* __restrict__ flag) {
  const int Do = D / 2, Ho = H / 2, Wo = W / 2;
  const long long cells_o = (long long)Do * Ho * Wo, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * cells_o) return;
  const int b = (int)(i / cells_o);
  const int c = (int)(i - (long long)b * cells_o);
  const int xo = c % Wo, yo = (c / Wo) % Ho, zo = c / (Wo * Ho);
  const int32_t* in = index_in + (long long)b * D * H * W;
  int any = 0;
  for (int dz = -1; dz <= 1; ++dz) {
    const int z = 2 * zo + dz;
    if (z < 0 || z >= D) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int y = 2 * yo + dy;
      if (y < 0 || y >= H) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int x = 2 * xo + dx;
        if (x < 0 || x >= W) continue;
        any |= in[((long long)z * H + y) * W + x] >= 0;
      }
    }
  }
  flag[i] = any;
}

__global__ __launch_bounds__(256) void sp_down_emit(const int32_t* __restrict__ flag, const int32_t* __restrict__ rp, int B, int cells_o,
                                                    int cap_out, int32_t* __restrict__ index_out, int32_t* __restrict__ cell_out,
                                                    int32_t* __restrict__ count_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * cells_o) return;
  const int b = (int)(i / cells_o);
  const int c = (int)(i - (long long)b * cells_o);
  const int32_t* r = rp + (long long)b * (cells_o + 1);
  int row = -1;
  if (flag[i]) {
    const int v = r[c];
    if (v < cap_out) {                                               // (always: cap_out = min(8 * cap_in, cells_o) bounds the set)
      row = b * cap_out + v;
      cell_out[row] = c;
    }
  }
  index_out[i] = row;
  if (c == 0) count_out[b] = r[cells_o] < cap_out ? r[cells_o] : cap_out;
}

struct TableArgs {
  const int32_t* index;      // the volume the taps look into [B][Di][Hi][Wi]
  const int32_t* cell;       // [B][cap] cells of the table's rows, in (Dr, Hr, Wr)
  const int32_t* count;      // [B]
  int32_t* table;            // [B * cap][27]
  int B, cap, Di, Hi, Wi, Hr, Wr, stride, transposed;
};

__device__ __forceinline__ bool tap_coord(int c, int k, int stride, int transposed, int n, int& out) {
  if (!transposed) {
    out = c * stride - 1 + k;
  } else {
    const int t = c + 1 - k;
    if (t < 0 || t % stride) return false;
    out = t / stride;
  }
  return out >= 0 && out < n;
}

__global__ __launch_bounds__(256) void sp_table(const TableArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.B * a.cap * 27) return;
  const long long row = i / 27;
  const int k = (int)(i - row * 27);
  int b;
  if (!row_active(a.count, a.cap, row, b)) return;
  int e = -1;
  const int c = a.cell[row];
  if (c >= 0) {
    const int x = c % a.Wr, y = (c / a.Wr) % a.Hr, z = c / (a.Wr * a.Hr);
    int zi, yi, xi;
    if (tap_coord(z, k / 9, a.stride, a.transposed, a.Di, zi) && tap_coord(y, (k / 3) % 3, a.stride, a.transposed, a.Hi, yi) &&
        tap_coord(x, k % 3, a.stride, a.transposed, a.Wi, xi))
      e = a.index[(((long long)b * a.Di + zi) * a.Hi + yi) * a.Wi + xi];
  }
  a.table[i] = e;
}

int grid_check(const char* who, int B, int cap, int D, int H, int W) {
  BEVF_REQUIRE(B > 0 && cap > 0 && D > 0 && H > 0 && W > 0, "%s: empty shape", who);
  BEVF_REQUIRE((long long)B * D * H * W < (1ll << 31), "%s: B * cells = %lld does not fit int32 (an index volume per level; no hash table)",
               who, (long long)B * D * H * W);
  BEVF_REQUIRE((long long)B * cap * 27 < (1ll << 31), "%s: B * capacity * 27 does not fit int32", who);
  return BEVF_OK;
}

unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int bevf_sparse_fill_index(const int64_t* coords, const int32_t* count, int B, int cap, int D, int H, int W, int32_t* index,
                                      int32_t* cell, void* stream) {
  if (int rc = grid_check("sparse_fill_index", B, cap, D, H, W)) return rc;
  BEVF_REQUIRE(coords && count && index && cell, "sparse_fill_index: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(index, 0xFF, (size_t)B * D * H * W * sizeof(int32_t), st) != hipSuccess) {       // -1: no row
    bevf_set_error("sparse_fill_index: memset failed");
    return BEVF_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(sp_fill_index, dim3(blocks_for((long long)B * cap)), dim3(256), 0, st, reinterpret_cast<const long long*>(coords),
                     count, B, cap, D, H, W, index, cell);
  return bevf_check_launch("bevf_sparse_fill_index");
}

extern "C" size_t bevf_sparse_down_work_bytes(int B, int D, int H, int W) {
  const size_t cells_o = (size_t)(D / 2) * (H / 2) * (W / 2);
  return ((size_t)B * cells_o + (size_t)B * (cells_o + 1)) * sizeof(int32_t) + 256;
}

extern "C" int bevf_sparse_down(const int32_t* index_in, int B, int D, int H, int W, int cap_out, int32_t* index_out, int32_t* cell_out,
                                int32_t* count_out, void* work, void* stream) {
  if (int rc = grid_check("sparse_down", B, cap_out, D, H, W)) return rc;
  BEVF_REQUIRE(index_in && index_out && cell_out && count_out && work, "sparse_down: null pointer");
  BEVF_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "sparse_down: grid dims (%d, %d, %d) must be even", D, H, W);
  const long long cells_o = (long long)(D / 2) * (H / 2) * (W / 2);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* flag = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(work) + 255) & ~uintptr_t(255));
  int32_t* rp = flag + (size_t)B * cells_o;
  hipLaunchKernelGGL(sp_down_mark, dim3(blocks_for(B * cells_o)), dim3(256), 0, st, index_in, B, D, H, W, flag);
  hipLaunchKernelGGL(scan_counts, dim3(B), dim3(1024), 0, st, flag, (int)cells_o, rp);
  hipLaunchKernelGGL(sp_down_emit, dim3(blocks_for(B * cells_o)), dim3(256), 0, st, flag, rp, B, (int)cells_o, cap_out, index_out, cell_out,
                     count_out);
  return bevf_check_launch("bevf_sparse_down");
}

extern "C" int bevf_sparse_table(const int32_t* index, const int32_t* cell, const int32_t* count, int B, int cap, int Di, int Hi, int Wi,
                                 int Dr, int Hr, int Wr, int stride, int transposed, int32_t* table, void* stream) {
  if (int rc = grid_check("sparse_table", B, cap, Di, Hi, Wi)) return rc;
  BEVF_REQUIRE(index && cell && count && table, "sparse_table: null pointer");
  BEVF_REQUIRE(Dr > 0 && Hr > 0 && Wr > 0 && (stride == 1 || stride == 2), "sparse_table: need a row grid and stride 1 or 2");
  TableArgs a;
  a.index = index; a.cell = cell; a.count = count; a.table = table;
  a.B = B; a.cap = cap; a.Di = Di; a.Hi = Hi; a.Wi = Wi; a.Hr = Hr; a.Wr = Wr; a.stride = stride; a.transposed = transposed != 0;
  hipLaunchKernelGGL(sp_table, dim3(blocks_for((long long)B * cap * 27)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return bevf_check_launch("bevf_sparse_table");
}
