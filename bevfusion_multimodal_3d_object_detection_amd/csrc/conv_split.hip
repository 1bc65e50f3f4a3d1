// fp32 implicit-GEMM convolution through three bf16 planes ("f32x3"), gfx950.
//
// Same GEMM view, tiling, A-operand addressing (ConvAWalker) and epilogue (conv_common.h) as conv_igemm.hip, but the multiply runs on
// v_mfma_f32_32x32x16_bf16 (16x the rate of v_mfma_f32_32x32x2_f32): every fp32 operand is split exactly into
//     x = hi + mid + lo,   hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)      (|residual| <~ 2^-25 |x|)
// and a product a*b is accumulated in fp32 as the six partial products that matter,
//     hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi          (dropped: mid*lo, lo*mid, lo*lo ~ 2^-24 |a*b|)
// so the result carries fp32-level error (measured against fp64 next to the exact-fp32 kernel in
// tests/test_gpu_split.py) without being bit-identical to an fp32 FMA chain.  It is an OPT-IN mode
// (engine.set_conv_mode("f32x3")); the default path stays exact fp32.
// Measured (MI355X, random data): 195-210 TF algorithmic on the 3x3 layers vs 135-146 for the exact kernel.  Halving the
// MFMA count in a what-if build showed the six products alone take ~2/3 of the time at ~1.77 PFLOP/s bf16 -- the chip
// holds ~1.7 GHz under this load -- so the scheme's ceiling is ~295 TF; the rest is staging (the split costs ~12 %).
//
// Activations stay fp32 in HBM and are split while they are staged into LDS (about 26 vector-ALU instructions per
// 4 elements; the bf16 MFMA leaves most of the vector issue slots free, unlike the fp32 MFMA).  Weights are split
// once by bevf_split_weights_f32x3 into [3][Cout][K] bf16 planes.
// LDS (single buffer, next K step prefetched in registers): per plane a row of a K step is 32 bf16 = 64 B = 4 chunks
// of 16 B; chunk c of row r sits at r*64 + ((c ^ ((r>>1)&3)) << 4), which makes the ds_read_b128 fragment reads
// (32 rows x one chunk per half-wave) bank-conflict free.  Lane half h of k-group g reads chunk 2g+h = k 16g+8h..+7,
// exactly the operand layout of v_mfma_f32_32x32x16_bf16.
#include "conv_common.h"

#include <cmath>

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void split3(const f32x4 v, u32x2& hi, u32x2& mid, u32x2& lo) {
  const bf16x4 h = __builtin_convertvector(v, bf16x4);
  const f32x4 r1 = v - __builtin_convertvector(h, f32x4);
  const bf16x4 m = __builtin_convertvector(r1, bf16x4);
  const f32x4 r2 = r1 - __builtin_convertvector(m, f32x4);
  const bf16x4 l = __builtin_convertvector(r2, bf16x4);
  hi = __builtin_bit_cast(u32x2, h);
  mid = __builtin_bit_cast(u32x2, m);
  lo = __builtin_bit_cast(u32x2, l);
}

__global__ __launch_bounds__(256) void split_weights(const float* __restrict__ w, __bf16* __restrict__ out, long long n) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const float x = w[i];
  const __bf16 h = (__bf16)x;
  const float r1 = x - (float)h;
  const __bf16 m = (__bf16)r1;
  const float r2 = r1 - (float)m;
  out[i] = h;
  out[n + i] = m;
  out[2 * n + i] = (__bf16)r2;
}

// The max-pruning bound pass (BOUND) is the same kernel on two planes (NPL = 2: hi, mid) and the three products
// hi*hi + hi*mid + mid*hi, with bound_epilogue below in place of the store: per row p and channel c it brackets the value the exact
// fp32 kernel would give, val -+ eps with eps = |a_p| * bound_g[c] + 2^-21 |val|, raises thr[group][c] (p.colmax) to max(val - eps, 0)
// and, unless it is a seed launch (p.flag == NULL: only every p.tm_stride-th row tile, thresholds only), flags every row that
// some channel cannot rule out: !(val + eps < thr) and !(val + eps <= 0), so that a NaN or infinite bound flags.  |a_p| comes
// from the squares summed while the row is staged (inflated, see the derivation); nothing is stored per (row, channel).
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void bound_epilogue(const ConvArgs& p, f32x16 (&acc)[WM / 32][WN / 32], const int m0, const int n0,
                                               const int m_hi, const int wm, const int wn, const int lane, const float* norms) {
  constexpr int MI = WM / 32, NI = WN / 32;
  const int h = lane >> 5, l31 = lane & 31;
  const int row_base = wm * WM + 4 * h, n_base = n0 + wn * WN;
  const int group = m0 / p.rows_per_group;
  const bool fast = (m0 + BM <= m_hi) && ((m0 + BM - 1) / p.rows_per_group == group);
  float na[MI][16];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) na[mi][r] = norms[row_base + mi * 32 + (r & 3) + 8 * (r >> 2)];
  unsigned fmask[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) fmask[mi] = 0u;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int n = n_base + ni * 32 + l31;
    const bool nok = n < p.Cout;
    const int nc = nok ? n : p.Cout - 1;
    float sc, sh;
    conv_scale_shift(p, nc, sc, sh);
    const float g = p.bound_g[nc];
    const float thr = fast ? __uint_as_float(__hip_atomic_load(&p.colmax[(size_t)group * p.Cout + nc], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0.f;
    float lbmax = 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float val = fmaf(acc[mi][ni][r], sc, sh);
        const float eps = fmaf(na[mi][r], g, fabsf(val) * 0x1p-21f);
        const float ub = val + eps;
        const float lb = fabsf(val) < __builtin_inff() ? val - eps : 0.f;     // an overflowed product bounds nothing from below
        if (fast) {
          lbmax = fmaxf(lbmax, lb);                                             // fmaxf drops a NaN
          if (p.flag && !(ub < thr) && !(ub <= 0.f)) fmask[mi] |= 1u << r;
        } else {
          const int m = m0 + row_base + mi * 32 + (r & 3) + 8 * (r >> 2);
          if (m < m_hi && nok) {
            uint32_t* const t = &p.colmax[(size_t)(m / p.rows_per_group) * p.Cout + n];
            const float th = __uint_as_float(__hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (lb > th) atomicMax(t, __float_as_uint(lb));
            if (p.flag && !(ub < th) && !(ub <= 0.f)) fmask[mi] |= 1u << r;
          }
        }
      }
    }
    if (fast) {
      lbmax = fmaxf(lbmax, __shfl_xor(lbmax, 32));
      if (h == 0 && nok && lbmax > thr) atomicMax(&p.colmax[(size_t)group * p.Cout + n], __float_as_uint(lbmax));
    }
  }
  if (!p.flag) return;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    unsigned f = fmask[mi];
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) f |= (unsigned)__shfl_xor((int)f, d);      // over the 32 channels of the half-wave
    const int m = m0 + row_base + mi * 32 + (l31 & 3) + 8 * ((l31 >> 2) & 3);
    if (l31 < 16 && ((f >> l31) & 1u) && m < m_hi) p.flag[m] = 1;
  }
}

// NPL = planes per operand: 3 = the six-product f32x3 convolution, 2 = hi and mid with three products (the bound pass).
template <int BM, int BN, int WM, int WN, int NPL = 3, bool BOUND = false>
__global__ __launch_bounds__(256) void conv_split(const ConvArgs p) {
  static_assert(NPL == 3 || (NPL == 2 && BOUND), "two planes are the bound pass");
  constexpr int WAVES_N = BN / WN;
  constexpr int MI = WM / 32, NI = WN / 32;
  constexpr int AP = BM / 32, BPJ = BN / 64;
  static_assert((BM / WM) * (BN / WN) == 4, "4 waves per workgroup");
  constexpr int A_PLANE = BM * 64, B_PLANE = BN * 64, B_BASE = NPL * A_PLANE;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* const ldsb = reinterpret_cast<char*>(lds);

  const int sid = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = (sid / p.tilesN) * (BOUND ? p.tm_stride : 1), tn = sid % p.tilesN;
  const int m_hi = p.M;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- A staging: thread owns fp32 chunk `chunk` (k = 4*chunk..+3) of rows srow + 32*j, through the walker of conv_common.h -------
  const int chunk = tid & 7, srow = tid >> 3;
  ConvAWalker<4, AP> aw;
  aw.init(p, m0 + srow, m_hi, chunk);
  // ---- B staging: thread owns 16-B chunk q (8 bf16) of rows brow + 64*j of each plane -----------------------
  const int bq = tid & 3, brow = tid >> 2;
  unsigned b_voff[BPJ];
#pragma unroll
  for (int j = 0; j < BPJ; ++j) {
    const int n = n0 + brow + 64 * j;
    b_voff[j] = n < p.Cout ? (unsigned)(((size_t)n * p.K) * 2 + bq * 16) : kOob;
  }
  const size_t plane_elems = (size_t)p.Cout * p.K;
  const __bf16* const wb = static_cast<const __bf16*>(p.w);
  const __amdgpu_buffer_rsrc_t rsrcB0 = buf_rsrc(wb), rsrcB1 = buf_rsrc(wb + plane_elems), rsrcB2 = buf_rsrc(wb + 2 * plane_elems);

  f32x4 ra[AP];
  u32x4 rb[NPL][BPJ];
  float ssq[AP];                                    // BOUND: this thread's part of |row|^2
#pragma unroll
  for (int j = 0; j < AP; ++j) ssq[j] = 0.f;
  auto load_tile = [&](int kstep) {                 // K step `kstep`, which the walker stands on
    aw.load(p, ra);
#pragma unroll
    for (int j = 0; j < BPJ; ++j) {
      rb[0][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrcB0, b_voff[j], (unsigned)kstep * 64u, 0);
      rb[1][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrcB1, b_voff[j], (unsigned)kstep * 64u, 0);
      if constexpr (NPL == 3) rb[2][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrcB2, b_voff[j], (unsigned)kstep * 64u, 0);
    }
  };

  // LDS addresses
  const int a_wr = srow * 64 + (((chunk >> 1) ^ ((srow >> 1) & 3)) << 4) + (chunk & 1) * 8;
  const int b_wr = B_BASE + brow * 64 + ((bq ^ ((brow >> 1) & 3)) << 4);
  const int h = lane >> 5, l31 = lane & 31;
  int a_rd[2], b_rd[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    a_rd[g] = (wm * WM + l31) * 64 + (((2 * g + h) ^ ((l31 >> 1) & 3)) << 4);
    b_rd[g] = B_BASE + (wn * WN + l31) * 64 + (((2 * g + h) ^ ((l31 >> 1) & 3)) << 4);
  }
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < AP; ++j) {
      u32x2 hi, mid, lo;
      split3(ra[j], hi, mid, lo);
      *reinterpret_cast<u32x2*>(ldsb + a_wr + j * 2048) = hi;
      *reinterpret_cast<u32x2*>(ldsb + a_wr + j * 2048 + A_PLANE) = mid;
      if constexpr (NPL == 3) *reinterpret_cast<u32x2*>(ldsb + a_wr + j * 2048 + 2 * A_PLANE) = lo;
      if constexpr (BOUND) ssq[j] = fmaf(ra[j][0], ra[j][0], fmaf(ra[j][1], ra[j][1], fmaf(ra[j][2], ra[j][2], fmaf(ra[j][3], ra[j][3], ssq[j]))));
    }
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
      for (int j = 0; j < BPJ; ++j) *reinterpret_cast<u32x4*>(ldsb + b_wr + pl * B_PLANE + j * 4096) = rb[pl][j];
  };

  f32x16 acc[MI][NI];
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto compute = [&](auto firstc) {
    constexpr bool first = decltype(firstc)::value;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      bf16x8 a[NPL][MI], b[NPL][NI];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          a[pl][mi] = *reinterpret_cast<const bf16x8*>(ldsb + a_rd[g] + pl * A_PLANE + mi * 2048);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          b[pl][ni] = *reinterpret_cast<const bf16x8*>(ldsb + b_rd[g] + pl * B_PLANE + ni * 2048);
      }
      // small partial products first: (hi,lo) (lo,hi) (mid,mid) (hi,mid) (mid,hi) (hi,hi)
      // (two planes: the last three)
      constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
      constexpr int T0 = NPL == 3 ? 0 : 3;
#pragma unroll
      for (int t = T0; t < 6; ++t)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA[t]][mi], b[PB[t]][ni],
                                                                  first && g == 0 && t == T0 ? zero : acc[mi][ni], 0, 0, 0);
    }
  };

  // ---- K loop: single LDS buffer, the next step's operands are in flight in registers during the MFMAs ----
  const int KT = p.K / BK;
  load_tile(0);
  store_tile();
  __syncthreads();
  if (KT > 1) {
    aw.advance(p);
    load_tile(1);
  }
  __builtin_amdgcn_sched_barrier(0);
  compute(std::true_type{});
  for (int kt = 1; kt < KT; ++kt) {
    __syncthreads();                                // every wave has read step kt-1
    store_tile();
    __syncthreads();
    if (kt + 1 < KT) {
      aw.advance(p);
      load_tile(kt + 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    compute(std::false_type{});
  }
  if constexpr (BOUND) {
    // |a_p|: the 8 lanes that staged a row hold its squares; inflated by 2^-10 (the sum's and the root's roundings stay below 2^-14
    // relative at K <= 2^16) plus 2^-58, which stands for elements whose squares underflow
    __syncthreads();                                // every wave has read the last K step: the operand tiles are dead
#pragma unroll
    for (int j = 0; j < AP; ++j) {
      float s = ssq[j];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 4);
      if (chunk == 0) lds[srow + 32 * j] = fmaf(sqrtf(s), 1.f + 0x1p-10f, 0x1p-58f);
    }
    __syncthreads();
    bound_epilogue<BM, BN, WM, WN>(p, acc, m0, n0, m_hi, wm, wn, lane, lds);
  } else {
    conv_epilogue<float, BM, BN, WM, WN>(p, acc, m0, n0, m_hi, wm, wn, lane);
  }
}

template <int BM, int BN, int WM, int WN>
int launch_split(ConvArgs a, hipStream_t st) {
  a.tilesM = (a.M + BM - 1) / BM;
  a.tilesN = (a.Cout + BN - 1) / BN;
  constexpr size_t lds_bytes = size_t(3) * (BM + BN) * 64;
  return bevf_launch("bevf_conv2d_nhwc_f32x3", conv_split<BM, BN, WM, WN>, dim3(a.tilesM * a.tilesN), dim3(256), lds_bytes, st, a);
}

template <int BM, int BN, int WM, int WN>
int launch_bound(ConvArgs a, int seed_stride, hipStream_t st) {
  const int tilesM = (a.M + BM - 1) / BM;
  a.tm_stride = seed_stride > 0 ? seed_stride : 1;
  a.tilesM = (tilesM + a.tm_stride - 1) / a.tm_stride;             // row tiles 0, stride, 2 * stride, ...
  a.tilesN = (a.Cout + BN - 1) / BN;
  constexpr size_t lds_bytes = size_t(2) * (BM + BN) * 64;
  return bevf_launch("bevf_conv2d_bound_f32x2", conv_split<BM, BN, WM, WN, 2, true>, dim3(a.tilesM * a.tilesN), dim3(256), lds_bytes, st, a);
}

}  // namespace

extern "C" int bevf_conv2d_bound_f32x2(const bevf_conv_desc* d, const float* bound_g, int32_t* flag, int seed_stride, void* stream) {
  ConvArgs a;
  if (const int rc = conv_args_from_desc(d, "conv bound", 4, 2, &a)) return rc;
  BEVF_REQUIRE(d->colmax && bound_g && d->rows_per_group > 0 && d->relu, "conv bound: needs thresholds (colmax), bound_g, rows_per_group > 0 and relu");
  BEVF_REQUIRE(!d->y && !d->res, "conv bound: stores no y and takes no residual");
  BEVF_REQUIRE((flag != nullptr) != (seed_stride > 0), "conv bound: a seed launch (seed_stride > 0) writes no flags, a main launch (0) needs them");
  BEVF_REQUIRE(((size_t)d->Cout * d->KH * d->KW * d->Cin * 2) % 16 == 0, "conv bound: plane size must be a multiple of 16 bytes");
  a.bound_g = bound_g;
  a.flag = flag;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (d->tile) {
    case 0: break;
    case 1: return launch_bound<128, 128, 64, 64>(a, seed_stride, st);
    case 4: return launch_bound<64, 64, 32, 32>(a, seed_stride, st);
    default: bevf_set_error("conv bound: unknown tile variant %d", d->tile); return BEVF_ERR_ARG;
  }
  if (d->Cout > 64 && a.M >= 4096) return launch_bound<128, 128, 64, 64>(a, seed_stride, st);
  return launch_bound<64, 64, 32, 32>(a, seed_stride, st);
}

extern "C" int bevf_split_weights_f32x3(const float* w, void* planes, size_t n, void* stream) {
  BEVF_REQUIRE(w && planes && n > 0, "split_weights: bad arguments");
  hipLaunchKernelGGL(split_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                     static_cast<__bf16*>(planes), (long long)n);
  return bevf_check_launch("bevf_split_weights_f32x3");
}

extern "C" int bevf_conv2d_nhwc_f32x3(const bevf_conv_desc* d, void* stream) {
  ConvArgs a;
  if (const int rc = conv_args_from_desc(d, "conv f32x3", 4, 2, &a)) return rc;
  BEVF_REQUIRE(d->y || d->colmax, "conv f32x3: needs y or colmax");
  BEVF_REQUIRE(!d->colmax || (d->rows_per_group > 0 && d->relu), "conv f32x3: colmax needs rows_per_group > 0 and relu (the max is taken over max(v, 0))");
  BEVF_REQUIRE(d->y_cs >= d->Cout, "conv f32x3: y_cs=%d < Cout=%d", d->y_cs, d->Cout);
  BEVF_REQUIRE(((size_t)d->Cout * d->KH * d->KW * d->Cin * 2) % 16 == 0, "conv f32x3: plane size must be a multiple of 16 bytes");
  const long long M = a.M;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (d->tile) {
    case 0: break;
    case 1: return launch_split<128, 128, 64, 64>(a, st);
    case 3: return launch_split<128, 64, 64, 32>(a, st);
    case 4: return launch_split<64, 64, 32, 32>(a, st);
    default: bevf_set_error("conv f32x3: unknown tile variant %d", d->tile); return BEVF_ERR_ARG;
  }
  const double wg128 = std::ceil(M / 128.0) * ((d->Cout + 127) / 128);
  if (d->Cout > 64 && wg128 >= 768) return launch_split<128, 128, 64, 64>(a, st);
  if (std::ceil(M / 128.0) * ((d->Cout + 63) / 64) >= 1024) return launch_split<128, 64, 64, 32>(a, st);
  return launch_split<64, 64, 32, 32>(a, st);
}
