// Transposed convolution with kernel = stride (nn.ConvTranspose2d(k = s, stride = s), the FPN neck's upsampling) on NHWC maps, gfx950.
//
//   y[n][s*h + i][s*w + j][co] = act( (sum_ci x[n][h][w][ci] * W[ci][co][i][j]) * scale[co] + shift[co] )
//
//   GEMM view:  C[M = N*H*W pixels][N' = s*s*Cout] = X[M][K = Cin] * Wp^T[K][N'],  n' = (i*s + j)*Cout + co
//   One launch: the GEMM, folded BN, ReLU and the scatter of row m's s*s channel runs to its s*s output pixels.  There is no
//   [M][N'] intermediate and no shuffle pass; y may be a channel slice of a wider map (y_cs), so a concat costs nothing.
//
// Workgroup = 256 threads = 4 waves, tile 128 pixels x 128 n' (N' is always a multiple of 128: s*s >= 4, Cout % 32 == 0), wave
// tile 64 x 64 from 32x32 MFMA tiles.  Staging, LDS layout and swizzle, fragment reads and the double-buffered K loop are those of
// conv_igemm.hip (a K step = 8 chunks of 16 B per row) -- as a copy without the filter-tap walk: conv_tile's text is pinned by that
// kernel's bit and timing tests ("Deviation"), and the operand order below differs inside its innermost loop; a fix to
// the loop there belongs here too.  The MFMA operands are SWAPPED against that kernel: the weight rows go in
// as the A operand and the pixel rows as B, so that in the accumulator C[i][j] the lane index j = lane & 31 is the PIXEL and the
// register index i = (r & 3) + 8*(r >> 2) + 4*(lane >> 5) the output channel.  A lane then holds 16 channels of one output pixel.
// The pack step orders the weight rows of each 32-channel group so that those 16 are two runs of 8 consecutive channels
// (row i <-> channel deconv_row_channel(i)): the lane stores them as 2 x 32 B (fp32) or 2 x 16 B (bf16) with 16-byte stores, and
// the two lane halves of a pixel together write 128 / 64 contiguous bytes.  A 32-row group lies inside one tap (i, j), so the
// tap and the channel base are wave-uniform: they become the store's scalar offset, the lane offset is the pixel's and is
// computed once per tile.
#include "conv_common.h"

#include <type_traits>

namespace {

struct DeconvArgs {
  const void* x;
  const void* w;
  const float* scale;
  const float* shift;
  void* y;
  int N, H, W, Cin, x_cs, Cout, y_cs, s, relu;
  int M, KT, Kp, tilesN;
  unsigned y_bytes;
  unsigned div_hw_mul, div_hw_sh, div_w_mul, div_w_sh, div_co_mul, div_co_sh;
};

// Channel (within its group of 32) whose weights sit in row i of the packed group: i = 8q + 4h + t -> 16*(q >> 1) + 8h + 4*(q & 1) + t.
// With the accumulator map above, lane half h holds channels 8h..8h+7 in registers 0..7 and 16+8h..16+8h+7 in registers 8..15.
__host__ __device__ constexpr int deconv_row_channel(int i) {
  return 16 * (i >> 4) + 8 * ((i >> 2) & 1) + 4 * ((i >> 3) & 1) + (i & 3);
}

constexpr int DBM = 128, DBN = 128;

template <typename T>
__global__ __launch_bounds__(256) void deconv_kernel(const DeconvArgs p) {
  constexpr int ES = (int)sizeof(T), EPC = 16 / ES, BKE = 8 * EPC;
  constexpr bool kF32 = std::is_same<T, float>::value;
  constexpr int AP = DBM / 32, BP = DBN / 32;
  constexpr int A_BYTES = DBM * BK * 4, B_BYTES = DBN * BK * 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* const ldsb = reinterpret_cast<char*>(lds);              // [A0][A1][B0][B1]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int sid = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (sid / p.tilesN) * DBM, n0 = (sid % p.tilesN) * DBN;

  // ---- staging: thread owns 16-B chunk `chunk` of pixel rows / weight rows srow + 32*j ----
  const int chunk = tid & 7, srow = tid >> 3;
  unsigned a_voff[AP], a_last[AP], b_voff[BP];
  const bool tail_dead = (p.KT - 1) * BKE + chunk * EPC >= p.Cin;   // bf16, Cin % 64 == 32: the last K step's upper half is padding
#pragma unroll
  for (int j = 0; j < AP; ++j) {
    const int m = m0 + srow + 32 * j;
    a_voff[j] = m < p.M ? (unsigned)((m * p.x_cs + chunk * EPC) * ES) : kOob;
    a_last[j] = tail_dead ? kOob : a_voff[j];
  }
#pragma unroll
  for (int j = 0; j < BP; ++j) b_voff[j] = (unsigned)(((n0 + srow + 32 * j) * p.Kp + chunk * EPC) * ES);
  const __amdgpu_buffer_rsrc_t rsrcA = buf_rsrc(p.x);
  const __amdgpu_buffer_rsrc_t rsrcB = buf_rsrc(p.w);

  f32x4 ra[AP], rb[BP];
  auto load_tile = [&](int kt) {
    const unsigned so = (unsigned)kt * 128u;
    if (kt == p.KT - 1) {
#pragma unroll
      for (int j = 0; j < AP; ++j) ra[j] = buf_load16(rsrcA, a_last[j], so);
    } else {
#pragma unroll
      for (int j = 0; j < AP; ++j) ra[j] = buf_load16(rsrcA, a_voff[j], so);
    }
#pragma unroll
    for (int j = 0; j < BP; ++j) rb[j] = buf_load16(rsrcB, b_voff[j], so);
  };

  // LDS: row r, 16-B chunk c at r*128 + ((c ^ ((r>>1)&7)) << 4), as in conv_igemm.hip
  const int wr_off = srow * 128 + ((chunk ^ ((srow >> 1) & 7)) << 4);
  const int h = lane >> 5, l31 = lane & 31;
  int a_rd[4], b_rd[4];
  {
    const int ra_row = wm * 64 + l31, rb_row = wn * 64 + l31;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      a_rd[g] = ra_row * 128 + (((2 * g + h) ^ ((ra_row >> 1) & 7)) << 4);
      b_rd[g] = 2 * A_BYTES + rb_row * 128 + (((2 * g + h) ^ ((rb_row >> 1) & 7)) << 4);
    }
  }
  auto store_tile = [&](auto bufc) {
    constexpr int buf = decltype(bufc)::value;
#pragma unroll
    for (int j = 0; j < AP; ++j) *reinterpret_cast<f32x4*>(ldsb + wr_off + buf * A_BYTES + j * 4096) = ra[j];
#pragma unroll
    for (int j = 0; j < BP; ++j) *reinterpret_cast<f32x4*>(ldsb + wr_off + 2 * A_BYTES + buf * B_BYTES + j * 4096) = rb[j];
  };

  f32x16 acc[2][2];                                   // [ni][mi]: rows = channels of group ni, columns = pixels of group mi
  auto compute = [&](auto bufc, auto firstc) {
    constexpr int buf = decltype(bufc)::value;
    constexpr bool first = decltype(firstc)::value;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x4 a[2], b[2], an[2], bn[2];
    auto rd = [&](int g, f32x4 (&fa)[2], f32x4 (&fb)[2]) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) fa[mi] = *reinterpret_cast<const f32x4*>(ldsb + a_rd[g] + buf * A_BYTES + mi * 4096);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) fb[ni] = *reinterpret_cast<const f32x4*>(ldsb + b_rd[g] + buf * B_BYTES + ni * 4096);
    };
    rd(0, a, b);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (g < 3) rd(g + 1, an, bn);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (kF32) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
              acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[ni][s], a[mi][s], first && g == 0 && s == 0 ? zero : acc[ni][mi], 0, 0, 0);
      } else {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
            acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, b[ni]), __builtin_bit_cast(bf16x8, a[mi]),
                                                                  first && g == 0 ? zero : acc[ni][mi], 0, 0, 0);
      }
      if (g < 3) {
#pragma unroll
        for (int i = 0; i < 2; ++i) { a[i] = an[i]; b[i] = bn[i]; }
      }
    }
  };

  // ---- K loop (conv_igemm.hip's): loads of step t+1 ahead of the MFMAs of step t, one barrier per step ----
  const int KT = p.KT;
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  using First = std::true_type;
  using Later = std::false_type;
  load_tile(0);
  store_tile(B0{});
  __syncthreads();
  auto two_steps = [&](auto firstc, const int kt) {
    load_tile(kt + 1);
    __builtin_amdgcn_sched_barrier(0);
    compute(B0{}, firstc);
    __builtin_amdgcn_sched_barrier(0);
    store_tile(B1{});
    __syncthreads();
    const bool more = kt + 2 < KT;
    if (more) load_tile(kt + 2);
    __builtin_amdgcn_sched_barrier(0);
    compute(B1{}, Later{});
    __builtin_amdgcn_sched_barrier(0);
    if (more) store_tile(B0{});
    __syncthreads();
  };
  int kt = 0;
  if (KT >= 2) {
    two_steps(First{}, 0);
    kt = 2;
  } else {
    compute(B0{}, First{});
    kt = 1;
  }
  for (; kt + 2 <= KT; kt += 2) two_steps(Later{}, kt);
  if (kt < KT) compute(B0{}, Later{});

  // ---- epilogue: lane = one input pixel; per 32-row group one tap and 16 channels in two runs of 8 ----
  const int sW = p.s * p.W, sH = p.s * p.H, HW = p.H * p.W;
  unsigned y_pix[2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int m = m0 + wm * 64 + mi * 32 + l31;
    if (m < p.M) {
      const int n = div_by(m, p.div_hw_mul, p.div_hw_sh), r = m - n * HW;
      const int hh = div_by(r, p.div_w_mul, p.div_w_sh), ww = r - hh * p.W;
      y_pix[mi] = (unsigned)((((n * sH + p.s * hh) * sW + p.s * ww) * p.y_cs + 8 * h) * ES);
    } else {
      y_pix[mi] = kOob;                               // out of the descriptor's range: the store is dropped
    }
  }
  const __amdgpu_buffer_rsrc_t ry = buf_rsrc(static_cast<const char*>(p.y), p.y_bytes);
  const bool relu = p.relu != 0;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int nb = n0 + wn * 64 + ni * 32;            // wave-uniform
    const int tap = div_by(nb, p.div_co_mul, p.div_co_sh), co0 = nb - tap * p.Cout;
    const int ti = tap / p.s, tj = tap - ti * p.s;
    const unsigned so = (unsigned)(((ti * sW + tj) * p.y_cs + co0) * ES);
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = co0 + 8 * h + (r & 7) + 16 * (r >> 3);
      sc[r] = p.scale ? p.scale[c] : 1.f;
      sh[r] = p.shift ? p.shift[c] : 0.f;
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float t = fmaf(acc[ni][mi][r], sc[r], sh[r]);
        v[r] = relu ? fmaxf(t, 0.f) : t;
      }
      if constexpr (kF32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 o = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ry, y_pix[mi] + (unsigned)((q & 1) * 16 + (q >> 1) * 64), so, 0);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[8 * q + e];
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ry, y_pix[mi] + (unsigned)(q * 32), so, 0);
        }
      }
    }
  }
}

// W (Cin, Cout, s, s) fp32, as nn.ConvTranspose2d holds it -> rows n' = tap*Cout + 32*group + i of Kp elements, zero past Cin.
template <typename T>
__global__ void deconv_pack_kernel(const float* __restrict__ w, T* __restrict__ out, int Cin, int Cout, int s, int Kp, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % Kp);
  const int row = (int)(idx / Kp);
  const int tap = row / Cout, rc = row - tap * Cout;
  const int co = (rc & ~31) + deconv_row_channel(rc & 31);
  out[idx] = k < Cin ? (T)w[((size_t)k * Cout + co) * (s * s) + tap] : (T)0.f;
}

static int deconv_kp(int Cin, int es) {
  const int bke = 128 / es;
  return (Cin + bke - 1) / bke * bke;
}

#define DECONV_UNSUPPORTED(cond, ...)   \
  do {                                  \
    if (!(cond)) {                      \
      bevf_set_error(__VA_ARGS__);      \
      return BEVF_ERR_UNSUPPORTED;      \
    }                                   \
  } while (0)

// The shape rules, shared by the launch and the pack entry points.
static int deconv_check_shape(const char* who, int Cin, int Cout, int s) {
  DECONV_UNSUPPORTED(s == 2 || s == 4, "%s: s=%d unsupported (2 or 4; s = 1 is a 1x1 convolution)", who, s);
  DECONV_UNSUPPORTED(Cin > 0 && Cin % 32 == 0, "%s: Cin=%d must be a positive multiple of 32", who, Cin);
  DECONV_UNSUPPORTED(Cout > 0 && Cout % 32 == 0, "%s: Cout=%d must be a positive multiple of 32", who, Cout);
  return BEVF_OK;
}

template <typename T>
int deconv_entry(const bevf_deconv_desc* d, void* stream) {
  constexpr int ES = (int)sizeof(T);
  const char* who = ES == 4 ? "deconv f32" : "deconv bf16";
  BEVF_REQUIRE(d && d->x && d->w && d->y, "%s: null x/w/y", who);
  BEVF_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "%s: empty shape", who);
  if (const int rc = deconv_check_shape(who, d->Cin, d->Cout, d->s)) return rc;
  DECONV_UNSUPPORTED(d->x_cs >= d->Cin && d->x_cs % 4 == 0 && (d->x_cs * ES) % 16 == 0, "%s: x_cs=%d must be >= Cin and a multiple of %d", who,
                     d->x_cs, ES == 4 ? 4 : 8);
  DECONV_UNSUPPORTED(d->y_cs >= d->Cout && (d->y_cs * ES) % 16 == 0, "%s: y_cs=%d must be >= Cout and a multiple of %d", who, d->y_cs,
                     16 / ES);
  DECONV_UNSUPPORTED(bevf_aligned16(d->x) && bevf_aligned16(d->w) && bevf_aligned16(d->y), "%s: x / w / y must be 16-byte aligned", who);
  const long long M = (long long)d->N * d->H * d->W;
  const long long x_elems = M * d->x_cs, y_elems = M * d->s * d->s * d->y_cs;
  DECONV_UNSUPPORTED(x_elems < (1ll << 31) && y_elems < (1ll << 31), "%s: N*H*W*x_cs and N*sH*sW*y_cs must stay below 2^31 (32-bit offsets)",
                     who);
  // the offsets are BYTE offsets: the rule above in bytes
  DECONV_UNSUPPORTED(x_elems * ES < (1ll << 31) && y_elems * ES < (1ll << 31), "%s: input / output maps must stay below 2 GiB (32-bit byte offsets)",
                     who);
  DeconvArgs a;
  a.x = d->x; a.w = d->w; a.scale = d->scale; a.shift = d->shift; a.y = d->y;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.x_cs = d->x_cs; a.Cout = d->Cout; a.y_cs = d->y_cs; a.s = d->s; a.relu = d->relu;
  a.M = (int)M;
  a.Kp = deconv_kp(d->Cin, ES);
  a.KT = a.Kp / (128 / ES);
  const long long np = (long long)d->s * d->s * d->Cout;
  DECONV_UNSUPPORTED(np * a.Kp * ES < (1ll << 31), "%s: packed weights must stay below 2 GiB", who);
  a.tilesN = (int)(np / DBN);
  a.y_bytes = (unsigned)(((M * d->s * d->s - 1) * d->y_cs + d->Cout) * ES);
  div_make(d->H * d->W, &a.div_hw_mul, &a.div_hw_sh);
  div_make(d->W, &a.div_w_mul, &a.div_w_sh);
  div_make(d->Cout, &a.div_co_mul, &a.div_co_sh);
  const long long tiles = (M + DBM - 1) / DBM * a.tilesN;
  DECONV_UNSUPPORTED(tiles < (1ll << 31), "%s: too many tiles", who);
  constexpr size_t lds_bytes = size_t(2) * (DBM + DBN) * BK * sizeof(float);
  return bevf_launch(ES == 4 ? "bevf_deconv_nhwc_f32" : "bevf_deconv_nhwc_bf16", deconv_kernel<T>, dim3((unsigned)tiles), dim3(256), lds_bytes,
                     static_cast<hipStream_t>(stream), a);
}

template <typename T>
int deconv_pack_entry(const float* w, void* out, int Cin, int Cout, int s, void* stream) {
  const char* who = sizeof(T) == 4 ? "deconv_pack f32" : "deconv_pack bf16";
  BEVF_REQUIRE(w && out, "%s: null w/out", who);
  if (const int rc = deconv_check_shape(who, Cin, Cout, s)) return rc;
  const int Kp = deconv_kp(Cin, (int)sizeof(T));
  const size_t total = (size_t)s * s * Cout * Kp;
  hipLaunchKernelGGL(deconv_pack_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                     static_cast<T*>(out), Cin, Cout, s, Kp, total);
  return bevf_check_launch(who);
}

}  // namespace

extern "C" size_t bevf_deconv_pack_elems(int Cin, int Cout, int s, int bf16) {
  if (Cin <= 0 || Cout <= 0 || s <= 0) return 0;
  return (size_t)s * s * Cout * deconv_kp(Cin, bf16 ? 2 : 4);
}
extern "C" int bevf_deconv_pack_f32(const float* w, float* out, int Cin, int Cout, int s, void* stream) {
  return deconv_pack_entry<float>(w, out, Cin, Cout, s, stream);
}
extern "C" int bevf_deconv_pack_bf16(const float* w, void* out, int Cin, int Cout, int s, void* stream) {
  return deconv_pack_entry<__bf16>(w, out, Cin, Cout, s, stream);
}
extern "C" int bevf_deconv_nhwc_f32(const bevf_deconv_desc* d, void* stream) { return deconv_entry<float>(d, stream); }
extern "C" int bevf_deconv_nhwc_bf16(const bevf_deconv_desc* d, void* stream) { return deconv_entry<__bf16>(d, stream); }
