// Sparse 3x3x3 convolution over the active rows of a level: an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact
// fp32: a k-ordered fmaf chain, like conv_igemm.hip) whose A rows are fetched through a neighbour table (sparse_index.hip).
//   sparse_conv   output stationary: a workgroup owns SP_BM = 128 output rows x Cout (32 rows per wave), K runs over 27 taps x Cin in steps of 32
//                 channels.  A rows come through a raw buffer descriptor: an absent neighbour (-1) is the out-of-range offset kOob and
//                 reads as zero.  A tap that no row of the tile uses is skipped (one flag per tap in LDS: the same for every wave).
//                 Epilogue: y = acc * scale + shift, ReLU (eval: folded BatchNorm), or the raw sums (train).  The data gradient is
//                 the same kernel: x = dy, the input-side table, weights packed [tap][Cout][Cin].
//   sparse_wgrad  dW[tap] = sum over rows of x[table[row][tap]]^T dy[row]: workgroup = (row chunk, tap), MFMA over 32-row steps with
//                 M = Cin and N = Cout, one fp32 partial per chunk, then a fixed-order sum into the torch layout [Cout][Cin][3][3][3].
// Rows are `cap` slots per frame, active while slot < count[b] (device memory); grids are sized by capacity and a tile with no
// active row returns at once.  No atomics: two launches give identical bits.
#include "conv_common.h"

namespace {

constexpr int SP_BM = 128;               // output rows per workgroup tile of sparse_conv (tests/test_gpu_sparse_lidar.py states it)
constexpr int APITCH = SP_BM + 1;        // A tile in LDS is [32 channels][SP_BM rows + 1]: fragment reads and staging writes spread over banks
constexpr int WG_ROWS = 32;              // rows per K step of sparse_wgrad
constexpr int WG_CHUNKS = 32;            // row chunks = partial sums per tap

struct SpConvArgs {
  const float* x;                        // [rows_in][Cin]
  const int32_t* table;                  // [B * cap][27] rows of x, -1 = absent
  const int32_t* count;                  // [B]
  const float* w;                        // [27][Cin][Cout]
  const float* scale;
  const float* shift;
  float* y;                              // [B * cap][Cout]
  int B, cap, Cin, Cout, relu;
  unsigned x_bytes;
};

// does any of the rows [r0, r0 + n) hold an active slot?  The same scalar loop in every thread: the answer is workgroup-uniform.
__device__ __forceinline__ bool tile_any_active(const int32_t* __restrict__ count, int B, int cap, long long r0, int n) {
  const long long total = (long long)B * cap;
  if (r0 >= total) return false;
  const long long r1 = r0 + n - 1 < total - 1 ? r0 + n - 1 : total - 1;
  const int b0 = (int)(r0 / cap), b1 = (int)(r1 / cap);
  bool any = false;
  for (int b = b0; b <= b1; ++b) {
    const int lo = b == b0 ? (int)(r0 - (long long)b0 * cap) : 0;
    any |= count[b] > lo;
  }
  return any;
}

__device__ __forceinline__ bool slot_active(const int32_t* __restrict__ count, int B, int cap, long long row) {
  if (row >= (long long)B * cap) return false;
  const int b = (int)(row / cap);
  return (int)(row - (long long)b * cap) < count[b];
}

template <int NT>                        // Cout / 32
__global__ __launch_bounds__(256) void sparse_conv(const SpConvArgs p) {
  __shared__ int tab_s[SP_BM * 27];
  __shared__ int act_s[SP_BM];
  __shared__ int used_s[27];
  __shared__ float As[32 * APITCH];
  __shared__ __attribute__((aligned(16))) float Bs[32 * NT * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long r0 = (long long)blockIdx.x * SP_BM;
  if (!tile_any_active(p.count, p.B, p.cap, r0, SP_BM)) return;
  if (tid < SP_BM) act_s[tid] = slot_active(p.count, p.B, p.cap, r0 + tid);
  __syncthreads();
  for (int i = tid; i < SP_BM * 27; i += 256) tab_s[i] = act_s[i / 27] ? p.table[r0 * 27 + i] : -1;
  __syncthreads();
  if (tid < 27) {
    int u = 0;
    for (int r = 0; r < SP_BM; ++r) u |= tab_s[r * 27 + tid] >= 0;
    used_s[tid] = u;
  }
  __syncthreads();

  // wave w owns rows 32 w .. 32 w + 31 of the tile and all NT column tiles: every B fragment read from LDS feeds four waves
  const int h = lane >> 5, l31 = lane & 31;
  const int chunk = tid & 7, arow = tid >> 3;                          // staging: 16-byte chunk `chunk` of rows arow + 32 q
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.x, p.x_bytes);
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  for (int tap = 0; tap < 27; ++tap) {
    if (!used_s[tap]) continue;                                        // the same LDS word in every thread: uniform
    unsigned off[SP_BM / 32];
#pragma unroll
    for (int q = 0; q < SP_BM / 32; ++q) {
      const int e = tab_s[(arow + 32 * q) * 27 + tap];
      off[q] = e >= 0 ? (unsigned)e * (unsigned)(p.Cin * 4) + chunk * 16 : kOob;
    }
    for (int c0 = 0; c0 < p.Cin; c0 += 32) {
      f32x4 av[SP_BM / 32], bv[NT];
#pragma unroll
      for (int q = 0; q < SP_BM / 32; ++q) av[q] = buf_load16(rx, off[q], (unsigned)(c0 * 4));
      const float* wb = p.w + ((size_t)tap * p.Cin + c0) * p.Cout;    // 32 x Cout floats, contiguous
#pragma unroll
      for (int j = 0; j < NT; ++j) bv[j] = *reinterpret_cast<const f32x4*>(wb + (j * 256 + tid) * 4);
      __syncthreads();                                                 // the previous step's fragment reads are done
#pragma unroll
      for (int q = 0; q < SP_BM / 32; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) As[(chunk * 4 + j) * APITCH + arow + 32 * q] = av[q][j];
#pragma unroll
      for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4*>(Bs + (j * 256 + tid) * 4) = bv[j];
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const int k = 2 * kk + h;
        const float a = As[k * APITCH + wave * 32 + l31];
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[k * (NT * 32) + j * 32 + l31], acc[j], 0, 0, 0);
      }
    }
  }
  // C[i][j]: j = lane & 31 (channel), i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (row of the wave's 32)
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = j * 32 + l31;
    const float sc = p.scale ? p.scale[n] : 1.f, sh = p.shift ? p.shift[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (!act_s[rl]) continue;
      float v = (p.scale || p.shift) ? fmaf(acc[j][r], sc, sh) : acc[j][r];
      if (p.relu) v = fmaxf(v, 0.f);
      p.y[(size_t)(r0 + rl) * p.Cout + n] = v;
    }
  }
}

struct SpWgradArgs {
  const float* x;                        // [rows_in][Cin]
  const float* dy;                       // [B * cap][Cout]
  const int32_t* table;                  // [B * cap][27]
  const int32_t* count;
  float* part;                           // [WG_CHUNKS][27][Cin][Cout]
  int B, cap, Cin, Cout;
  unsigned x_bytes, dy_bytes;
};

__global__ __launch_bounds__(256) void sparse_wgrad(const SpWgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];          // Xs [32][Cin], then dYs [32][Cout]
  __shared__ int e_s[WG_ROWS];
  __shared__ int any_s;
  float* Xs = lds;
  float* Ys = lds + WG_ROWS * p.Cin;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const int chunk = blockIdx.x, tap = blockIdx.y;
  const int MT = p.Cin >> 5, NT = p.Cout >> 5, tiles = MT * NT;
  const long long total = (long long)p.B * p.cap, ntile = (total + WG_ROWS - 1) / WG_ROWS;
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.x, p.x_bytes), rdy = buf_rsrc(p.dy, p.dy_bytes);
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const int xq = p.Cin >> 2, yq = p.Cout >> 2;                          // 16-byte chunks per row
  for (long long t = chunk; t < ntile; t += WG_CHUNKS) {
    const long long r0 = t * WG_ROWS;
    if (!tile_any_active(p.count, p.B, p.cap, r0, WG_ROWS)) continue;
    __syncthreads();                                                   // the previous step's reads of e_s / Xs / Ys are done
    if (tid < WG_ROWS) {
      const bool act = slot_active(p.count, p.B, p.cap, r0 + tid);
      const int e = act ? p.table[(r0 + tid) * 27 + tap] : -1;
      e_s[tid] = e;
      const unsigned long long m = __ballot(e >= 0);
      if (tid == 0) any_s = m != 0ull;
    }
    __syncthreads();
    if (!any_s) continue;                                              // no row of the step has this tap
    for (int q = tid; q < WG_ROWS * xq; q += 256) {
      const int r = q / xq, c = q - r * xq, e = e_s[r];
      const unsigned off = e >= 0 ? (unsigned)e * (unsigned)(p.Cin * 4) + c * 16 : kOob;
      *reinterpret_cast<f32x4*>(Xs + q * 4) = buf_load16(rx, off, 0);
    }
    for (int q = tid; q < WG_ROWS * yq; q += 256) {
      const int r = q / yq, c = q - r * yq;
      // a row without the tap contributes nothing, whatever its dy slot holds (inactive slots are never written)
      const unsigned off = e_s[r] >= 0 ? (unsigned)(r0 + r) * (unsigned)(p.Cout * 4) + c * 16 : kOob;
      *reinterpret_cast<f32x4*>(Ys + q * 4) = buf_load16(rdy, off, 0);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tl = wave + 4 * j;
      if (tl >= tiles) continue;
      const int mi = tl / NT, ni = tl - mi * NT;
#pragma unroll
      for (int kk = 0; kk < WG_ROWS / 2; ++kk) {
        const int k = 2 * kk + h;
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Xs[k * p.Cin + mi * 32 + l31], Ys[k * p.Cout + ni * 32 + l31], acc[j], 0, 0, 0);
      }
    }
  }
  float* out = p.part + ((size_t)chunk * 27 + tap) * p.Cin * p.Cout;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int tl = wave + 4 * j;
    if (tl >= tiles) continue;
    const int mi = tl / NT, ni = tl - mi * NT;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      out[(size_t)ci * p.Cout + ni * 32 + l31] = acc[j][r];
    }
  }
}

// dw [Cout][cin_real][27] (torch's Conv3d layout) = the chunks' partials [27][Cin][Cout] summed in chunk order
__global__ __launch_bounds__(256) void sparse_wgrad_finish(const float* __restrict__ part, int Cin, int Cout, int cin_real,
                                                           float* __restrict__ dw) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = 27 * Cin * Cout;
  if (i >= n) return;
  const int co = i % Cout, ci = (i / Cout) % Cin, tap = i / (Cout * Cin);
  if (ci >= cin_real) return;
  float s = 0.f;
  for (int c = 0; c < WG_CHUNKS; ++c) s += part[(size_t)c * n + i];
  dw[((size_t)co * cin_real + ci) * 27 + tap] = s;
}

int conv_check(const char* who, int B, int cap, long long rows_in, int Cin, int Cout) {
  BEVF_REQUIRE(B > 0 && cap > 0 && rows_in > 0, "%s: empty shape", who);
  BEVF_REQUIRE(Cin > 0 && Cin <= 128 && Cin % 32 == 0 && Cout > 0 && Cout <= 128 && Cout % 32 == 0,
               "%s: Cin=%d and Cout=%d must be multiples of 32 up to 128", who, Cin, Cout);
  BEVF_REQUIRE((long long)B * cap * 27 < (1ll << 31), "%s: B * capacity * 27 does not fit int32", who);
  BEVF_REQUIRE(rows_in * Cin * 4 < (1ll << 31) && (long long)B * cap * Cout * 4 < (1ll << 31),
               "%s: feature rows must stay below 2 GiB (32-bit buffer offsets)", who);
  return BEVF_OK;
}

}  // namespace

extern "C" int bevf_sparse_conv_f32(const float* x, const int32_t* table, const int32_t* count, const float* w, const float* scale,
                                    const float* shift, int B, int cap, int rows_in, int Cin, int Cout, int relu, float* y, void* stream) {
  if (int rc = conv_check("sparse_conv", B, cap, rows_in, Cin, Cout)) return rc;
  BEVF_REQUIRE(x && table && count && w && y, "sparse_conv: null pointer");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(w), "sparse_conv: x / w must be 16-byte aligned");
  SpConvArgs p;
  p.x = x; p.table = table; p.count = count; p.w = w; p.scale = scale; p.shift = shift; p.y = y;
  p.B = B; p.cap = cap; p.Cin = Cin; p.Cout = Cout; p.relu = relu;
  p.x_bytes = (unsigned)((long long)rows_in * Cin * 4);
  const dim3 grid((unsigned)(((long long)B * cap + SP_BM - 1) / SP_BM));
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (Cout / 32) {
    case 1: hipLaunchKernelGGL(sparse_conv<1>, grid, dim3(256), 0, st, p); break;
    case 2: hipLaunchKernelGGL(sparse_conv<2>, grid, dim3(256), 0, st, p); break;
    case 3: hipLaunchKernelGGL(sparse_conv<3>, grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL(sparse_conv<4>, grid, dim3(256), 0, st, p); break;
  }
  return bevf_check_launch("bevf_sparse_conv_f32");
}

extern "C" int bevf_sparse_conv_row_tile(void) { return SP_BM; }

extern "C" size_t bevf_sparse_wgrad_work_floats(int Cin, int Cout) { return (size_t)WG_CHUNKS * 27 * Cin * Cout + 64; }

extern "C" int bevf_sparse_conv_wgrad_f32(const float* x, const float* dy, const int32_t* table, const int32_t* count, int B, int cap,
                                          int rows_in, int Cin, int Cout, int cin_real, float* dw, float* work, void* stream) {
  if (int rc = conv_check("sparse_conv_wgrad", B, cap, rows_in, Cin, Cout)) return rc;
  BEVF_REQUIRE(x && dy && table && count && dw && work, "sparse_conv_wgrad: null pointer");
  BEVF_REQUIRE(cin_real > 0 && cin_real <= Cin, "sparse_conv_wgrad: cin_real=%d must be in 1..Cin", cin_real);
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(dy), "sparse_conv_wgrad: x / dy must be 16-byte aligned");
  SpWgradArgs p;
  p.x = x; p.dy = dy; p.table = table; p.count = count;
  p.part = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(work) + 255) & ~uintptr_t(255));
  p.B = B; p.cap = cap; p.Cin = Cin; p.Cout = Cout;
  p.x_bytes = (unsigned)((long long)rows_in * Cin * 4);
  p.dy_bytes = (unsigned)((long long)B * cap * Cout * 4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = (size_t)WG_ROWS * (Cin + Cout) * sizeof(float);
  hipLaunchKernelGGL(sparse_wgrad, dim3(WG_CHUNKS, 27), dim3(256), lds, st, p);
  hipLaunchKernelGGL(sparse_wgrad_finish, dim3((27 * Cin * Cout + 255) / 256), dim3(256), 0, st, p.part, Cin, Cout, cin_real, dw);
  return bevf_check_launch("bevf_sparse_conv_wgrad_f32");
}
