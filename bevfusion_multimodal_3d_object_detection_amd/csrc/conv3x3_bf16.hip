// bf16 direct convolution for the 3x3 / stride 1 / pad 1 layers on v_mfma_f32_16x16x32_bf16 (fp32 accumulate), gfx950.
//
// Why its own kernel (round 3): the implicit-GEMM template (conv_igemm.hip) was designed for the fp32 MFMA and is
// LDS-port-bound at the bf16 MFMA's 16x higher rate -- every K step re-stages a 128-byte A row per output pixel through
// registers and ds_write, and for a 3x3 layer the same input pixel is staged nine times (once per filter tap).  Here the
// reuse is explicit:
//   * a workgroup owns a 16x16 block of output pixels x CT output channels; per 32-channel chunk the 18x18-pixel input
//     patch is staged ONCE (LDS-DMA, `buffer_load ... lds`, zero fill for padding / image borders by out-of-range
//     offsets) and all nine taps read their fragments from it at shifted addresses: 7x less global->LDS traffic and no
//     ds_write at all;
//   * the filters are packed on the host side of the C-ABI (bevf_conv3x3_pack_bf16) into the exact MFMA fragment order,
//     one CT x 32 slice per (chunk, tap) step, so staging them is a straight LDS-DMA copy into a small ring and the
//     fragment reads are lane-linear (bank-conflict-free);
//   * the patch image is [pixel][4 x 16 B] with the 16-byte piece index XOR-swizzled by ((pixel >> 2) & 1) << 1: the
//     ds_read_b128 of a 16-pixel row segment (lane = pixel, lane>>4 = k group) then touches every bank exactly once in
//     each of the instruction's four lane groups, for every tap shift (MI355X_MICROARCH.md "LDS");
//   * C^T orientation: the MFMA's A operand is the filter fragment, B the pixels, so a lane ends up with 4 consecutive
//     output channels of one pixel -> 8-byte bf16x4 stores / residual loads instead of 2-byte ones;
//   * 64 or 128 accumulator registers per wave and 36-72 KB of LDS: two to four workgroups per CU, so one workgroup's
//     prologue / epilogue / barrier waits overlap the others' MFMAs.
// Every wait is written by hand (`s_waitcnt vmcnt(N)` + `s_barrier` in one asm): through __syncthreads() hipcc drains
// the LDS-DMA queue (vmcnt(0)) at every barrier.
//
// Code layout: the three kernels below are the same design cut three ways, and every stage they share is written once in the helpers
// that precede them (tile decode, patch / ring DMA, fragment addresses, the MFMA step, the nine taps, the step's wait count, the
// line epilogue).  A kernel body is the schedule: what is issued when, and what is waited for.
#include "conv_common.h"

#include <type_traits>
#include <utility>

namespace {

constexpr bool C3_AUTO_WIDE64 = true;                      // `tile = 0` with Cin = 64 takes the one-image kernel (tile = 5 forces it)
constexpr bool C3_AUTO_PERSIST = false;                    // `tile = 0` takes the persistent kernel (tile = 4 forces it)
constexpr int C3_AUTO_SHORTK = 1;                         // what `tile = 0` means for 64-channel tiles with Cin < 128 (1 | 2 | 3)
#ifndef C3_RB64
#define C3_RB64 8                                          // filter ring slots of the 64-channel / two-buffer kernels (C3Geo::RB)
#endif
#ifndef C3_RB128
#define C3_RB128 4                                         // ... of the 128-channel kernel
#endif

struct C3Args {
  const void* x;        // bf16 NHWC, channel stride x_cs
  const void* wp;       // packed filters: [ct][chunk][tap][CT/16][64 lanes][8 bf16]
  const float* scale;   // [Cout] or null
  const float* shift;
  const void* res;      // bf16 NHWC residual or null
  void* y;              // bf16 NHWC
  // (pad0 / pad1: no kernel reads them.  They keep the offsets the fields behind them have always had: hipcc groups the kernarg loads
  //  by offset, and without the two words the persistent kernel rebuilds a buffer-descriptor word in every step and spills one more SGPR.
  //  A property of this compiler, not of the design: they may go whenever that kernel's SGPR spills and s_mov count are checked again)
  int N, H, W, Cin, x_cs, pad0, y_cs, res_cs, relu;
  int TBY, TBX, pad1;   // blocks per image, of the launched kernel's block height x 16 pixels
  unsigned wbytes;      // size of the packed filter image
  unsigned long long* stamps;   // diagnostic builds of a run (bevf_debug_conv3x3_stamps): 4 x s_memtime per workgroup, else null
};

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* c3_lds_ptr;

constexpr int C3_PW = 18;                                 // patch width in pixels (block width 16 + halo)
constexpr int C3_PITCH = 20;                              // patch row pitch in the LDS image, pixels (see c3_frag_addrs)
// Every wave requests a quarter of both the filters and the patch.  (Tried: waves 0, 1 requesting only filters and waves 2, 3 only the
// patch, so that a filter wait never stands behind an HBM-latency patch piece in the in-order vmcnt queue -- 3-10 % SLOWER on every layer:
// issuing an LDS-DMA costs its wave 60-180 cycles, and two waves carrying all of one kind become the step's critical path.)
constexpr int C3_NSH = 4;                                 // waves sharing the DMA duty; a wave's `role` is its index

// CT = output channels per workgroup (64: waves 4 x 1, 128: waves 2 x 2; a wave always owns 64 channels).
// PB = patch buffers: 2 = the next 32-channel chunk is prefetched under the current one (two workgroups per CU);
//      1 = one buffer, FOUR workgroups per CU at BH = 16: occupancy instead of prefetch.
// BH = block height in pixel rows: 16 (16 x 16 = 256 pixels) or, for 64-channel tiles, 32 (512 pixels: a wave owns 8 rows instead of 4;
//      twice the MFMA work per tile, per barrier and per filter byte against the same fixed latencies -- for the short-K layers).
template <int CT, int PB, int BH> struct C3Geo {
  static constexpr int WN = CT / 64, WM = 4 / WN, MT = BH / WM, NT = 4;
  static constexpr int PH = BH + 2;                       // patch height
  static constexpr int PIXB = 64, ROWB = C3_PITCH * PIXB; // one 32-channel chunk of a pixel; bytes per patch row
  static constexpr int PPW = (PH * ROWB / 16 + 255) / 256;      // LDS-DMA pieces (64 slots of 16 B) per wave and patch chunk
  static constexpr int PATCH_BYTES = 4 * PPW * 1024;
  static constexpr int WSTEP = CT * 64;                   // bytes of filters per (chunk, tap) step
  static constexpr int FPW = (CT / 16) / C3_NSH;          // filter pieces per wave and step
  // ring slots; a step's filters are requested RB-1 steps ahead.  The depth is not for the filters (L2 hits): loads retire in order, so
  // a patch piece (HBM, 4-8k cycles under load) must land within RB-1 steps of its issue or the filter wait behind it stalls
  static constexpr int RB = (CT == 64 && PB == 2) ? C3_RB64 : (CT == 128 ? C3_RB128 : 3);
  static constexpr int LDS_BYTES = PB * PATCH_BYTES + RB * WSTEP;
  static constexpr int WG_PER_CU = (PB == 1 && BH == 16) ? 4 : 2;
  static constexpr bool RES_EARLY = CT == 64 && PB == 2 && BH == 16;  // residual requested in the prologue (32 registers; see the kernel)
};
// conv3x3_bf16_wide64: both 32-channel halves of a pixel side by side, the whole Cin = 64 patch in one image
struct C3GeoWide64 {
  static constexpr int CT = 64, MT = 4, NT = 4, BH = 16, PH = BH + 2, S = 18;
  static constexpr int PIXB = 128, ROWB = C3_PITCH * PIXB;          // 2560 bytes per patch row
  static constexpr int PPW = (PH * ROWB / 16 + 255) / 256;          // DMA pieces per wave: 12
  static constexpr int PATCH_BYTES = 4 * PPW * 1024;                // 49152
  static constexpr int WSTEP = CT * 64, FPW = (CT / 16) / C3_NSH, RB = 8;
  static constexpr int LDS_BYTES = PATCH_BYTES + RB * WSTEP;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t c3_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void c3_drain() { asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- tile id -> (channel tile, image, block row, block column): ct-major numbering, so the workgroups running together share one
//      filter slab in L2 ------------------------------------------------------------------------------------------------------------
struct C3Tile { int ct, n, by, bx; };
__device__ __forceinline__ C3Tile c3_decode(const C3Args& p, int t) {
  const int nsp = p.N * p.TBY * p.TBX;
  C3Tile r;
  r.ct = t / nsp;
  int sp = t - r.ct * nsp;
  r.bx = sp % p.TBX;
  sp /= p.TBX;
  r.by = sp % p.TBY;
  r.n = sp / p.TBY;
  return r;
}

// ---- patch staging: pieces J0 .. J1-1 of this wave for tile T's patch, channels from byte `soff` on, into the image at `buf`.
//      Instruction (4 j + role) fills 64 consecutive 16-byte slots; with SPP = PIXB / 16 slots per pixel, slot i = image pixel i / SPP
//      (rows of 20: 18 + 2 unused), channel half (i % SPP) >> 2, piece (i & 3) ^ swz(pixel): the swizzle sits on the SOURCE address, the
//      LDS image stays lane-linear.  Padding, image borders and a dead patch (`live` false) are out-of-range offsets: zero fill.  The
//      source offsets are recomputed at every call instead of living in registers across the K loop; OPAQUE keeps hipcc from hoisting
//      them out of it ---------------------------------------------------------------------------------------------------------------
template <int PIXB, int PH, int J0, int J1, bool OPAQUE>
__device__ __forceinline__ void c3_patch_dma(const C3Args& p, __amdgpu_buffer_rsrc_t rsx, const C3Tile& T, char* buf, int role, int lane,
                                             unsigned soff, bool live) {
  static_assert(PIXB == 64 || PIXB == 128, "one or two 32-channel halves per pixel");
  constexpr int SPP = PIXB / 16, LOG_SPP = PIXB == 64 ? 2 : 3;
  int l = lane;
  if constexpr (OPAQUE) asm volatile("" : "+v"(l));
  const int iy0 = (PH - 2) * T.by - 1, ix0 = 16 * T.bx - 1;
#pragma unroll
  for (int j = J0; j < J1; ++j) {
    const int i = (C3_NSH * j + role) * 64 + l;
    const int pix = i >> LOG_SPP, q = i & (SPP - 1), half = q >> 2, kg = (q & 3) ^ (((pix >> 2) & 1) << 1);
    const int py = (pix * 3277) >> 16, px = pix - py * C3_PITCH;         // pix / 20 for pix < 16384 / 4
    const int iy = iy0 + py, ix = ix0 + px;
    const bool ok = live && px < C3_PW && py < PH && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    const unsigned voff = ok ? (unsigned)((((T.n * p.H + iy) * p.W + ix) * p.x_cs + half * 32 + kg * 8) * 2) : kOob;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (c3_lds_ptr)(buf + (C3_NSH * j + role) * 1024), 16, voff, soff, 0, 0);
  }
}

// ---- filter ring: the image of a step is WSTEP contiguous bytes at `wofs` ((ct * S + s) * WSTEP); wave `role` copies pieces role,
//      role + 4, .. into the slot at `slot`.  Steps past the end read past num_records and arrive as zeros in a slot nobody reads --
template <int FPW>
__device__ __forceinline__ void c3_ring_dma(__amdgpu_buffer_rsrc_t rsw, char* slot, int role, int lane, unsigned wofs) {
#pragma unroll
  for (int i = 0; i < FPW; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (c3_lds_ptr)(slot + (role + C3_NSH * i) * 1024), 16, (unsigned)(lane * 16),
                                             wofs + (unsigned)((role + C3_NSH * i) * 1024), 0, 0);
}
template <int RB> __device__ __forceinline__ int c3_ring_ahead(int slot) {   // the slot RB-1 steps ahead
  const int ns = slot + RB - 1;
  return ns >= RB ? ns - RB : ns;
}
template <int RB> __device__ __forceinline__ int c3_ring_next(int slot) { return slot + 1 == RB ? 0 : slot + 1; }

// ---- fragment read addresses (bytes).  Image pixel (py, px) sits at slot (py * 20 + px) * SPP + (kg ^ swz), swz = 2 * (((py * 20 + px) >> 2) & 1)
//      = 2 * ((py & 1) ^ ((px >> 2) & 1)) because a row is 5 quads: the address of (row, tap column kw) is a per-lane term that depends on
//      kw and the row's PARITY only (6 registers) plus row * ROWB as an instruction immediate (the wave's first row `row0` is even) -----
template <int PIXB>
__device__ __forceinline__ void c3_frag_addrs(int (&xa)[3][2], int row0, int lane) {
  const int col = lane & 15, kgl = lane >> 4;
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      const int px = kw + col;
      xa[kw][par] = row0 * (C3_PITCH * PIXB) + px * PIXB + ((kgl ^ ((par ^ ((px >> 2) & 1)) << 1)) << 4);
    }
}

// ---- one step = tap T of one 32-channel chunk: NT filter fragments (lane-linear, `wb`), LIVE pixel-row fragments at the tap's shift in
//      the patch image `pb`, LIVE x NT MFMAs (mt outer, nt inner).  Rows LIVE .. MT-1 of the wave lie below the image and are skipped --
template <int T, int LIVE, int ROWB, int NT, int MT>
__device__ __forceinline__ void c3_mma(f32x4 (&acc)[NT][MT], const char* wb, const char* pb, const int (&xa)[3][2]) {
  constexpr int kh = T / 3, kw = T % 3;
  if constexpr (LIVE > 0) {
    bf16x8 wf[NT], xf[LIVE];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wf[nt] = *reinterpret_cast<const bf16x8*>(wb + nt * 1024);
#pragma unroll
    for (int mt = 0; mt < LIVE; ++mt) xf[mt] = *reinterpret_cast<const bf16x8*>(pb + xa[kw][(mt + kh) & 1] + (mt + kh) * ROWB);
#pragma unroll
    for (int mt = 0; mt < LIVE; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf[mt], acc[nt][mt], 0, 0, 0);
  }
}
template <int NT, int MT> __device__ __forceinline__ void c3_zero(f32x4 (&acc)[NT][MT]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- f(integral_constant<int, 0>) .. f(integral_constant<int, 8>): the nine taps of a chunk, each a compile-time constant ----------
template <class F, int... T> __device__ __forceinline__ void c3_taps(F&& f, std::integer_sequence<int, T...>) {
  (f(std::integral_constant<int, T>{}), ...);
}
template <class F> __device__ __forceinline__ void c3_nine_taps(F&& f) { c3_taps(f, std::make_integer_sequence<int, 9>{}); }

// ---- the wait at the end of step (tap) t.  Issue order inside a step: the FPW filter pieces of step s + D, then (PB = 2, taps
//      0 .. PPW-1) one piece of the NEXT chunk's patch.  Loads, DMAs and stores retire in order, so the count is what the wave has issued
//      AFTER the filters of step s + 1 (which left first thing in step s + 1 - D): FPW per later step and one patch piece in each of the
//      D steps whose tap is < PPW; everything younger stays in flight across the barrier.
//      Tap 8 must ALSO leave the next chunk's whole patch landed: nothing may stay in flight but what was issued after its last piece
//      (tap PPW-1), i.e. the filters of taps PPW .. 8.  (With a ring deeper than that the first count alone let patch pieces fly across
//      the chunk boundary: wrong pixels at full size only, where the DMA queue is long -- caught by the batch-invariance test of config 5,
//      not by the small-shape tests.)
//      The persistent kernel has more in its queue: `at_tap0` loads issued in tap 0 of this chunk after its DMAs (in flight by right in
//      the first D steps) and `before_tap0` stores issued just before the chunk (in its first D-1 steps) -----------------------------
constexpr int c3_step_vmcnt(int t, int D, int FPW, int PPW, int PB, int at_tap0 = 0, int before_tap0 = 0) {
  int c = (D - 1) * FPW;
  if (PB == 2) {
    for (int u = 0; u < D; ++u) c += ((t - u + 9) % 9) < PPW ? 1 : 0;
    if (t == 8 && c > (9 - PPW) * FPW) c = (9 - PPW) * FPW;
  }
  if (t <= D - 1 && t != 8) c += at_tap0;
  if (t <= D - 2 && t != 8) c += before_tap0;
  return c > 63 ? 63 : c;
}
// the counts of every (instantiation, tap) as the kernels had them before they shared this function
constexpr bool c3_vmcnt_are(const int (&want)[9], int D, int FPW, int PPW, int PB, int at_tap0 = 0, int before_tap0 = 0) {
  for (int t = 0; t < 9; ++t)
    if (c3_step_vmcnt(t, D, FPW, PPW, PB, at_tap0, before_tap0) != want[t]) return false;
  return true;
}
static_assert(C3_RB64 != 8 || c3_vmcnt_are({10, 10, 10, 10, 11, 12, 12, 11, 3}, 7, 1, 6, 2), "conv3x3_bf16<64, 2, 16>");
static_assert(c3_vmcnt_are({1, 1, 1, 1, 1, 1, 1, 1, 1}, 2, 1, 6, 1), "conv3x3_bf16<64, 1, 16>");
static_assert(c3_vmcnt_are({1, 1, 1, 1, 1, 1, 1, 1, 1}, 2, 1, 11, 1), "conv3x3_bf16<64, 1, 32>");
static_assert(C3_RB128 != 4 || c3_vmcnt_are({5, 6, 7, 7, 7, 7, 6, 5, 4}, 3, 2, 6, 2), "conv3x3_bf16<128, 2, 16>");
static_assert(c3_vmcnt_are({6, 6, 6, 6, 6, 6, 6, 6, 6}, 7, 1, 0, 1), "conv3x3_bf16_wide64<64>: no patch pieces in the loop");
static_assert(C3_RB64 != 8 || c3_vmcnt_are({10, 10, 10, 10, 11, 12, 12, 11, 3}, 7, 1, 6, 2, 0, 0), "conv3x3_bf16_persist<64>: inner chunk");
static_assert(C3_RB64 != 8 || c3_vmcnt_are({26, 26, 26, 26, 27, 28, 28, 11, 3}, 7, 1, 6, 2, 16, 0), "... last chunk");
static_assert(C3_RB64 != 8 || c3_vmcnt_are({26, 26, 26, 26, 27, 28, 12, 11, 3}, 7, 1, 6, 2, 0, 16), "... first chunk after an epilogue");
static_assert(C3_RB64 != 8 || c3_vmcnt_are({42, 42, 42, 42, 43, 44, 28, 11, 3}, 7, 1, 6, 2, 16, 16), "... both");
template <int CNT> __device__ __forceinline__ void c3_step_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CNT) : "memory");
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- output side (round 3, after layer1's in-kernel stamps and the wide64 experiment): whole 128-byte lines.  In the MFMA layout a
//      lane holds 4 channels of a pixel, so residual loads / output stores were 16 x 32-byte segments per instruction; that access
//      shape, not a latency, was what bound the short-K layers (layer1 483 -> 394 us with nothing else changed).  The epilogue
//      therefore transposes the accumulators through LDS in passes of RP pixel rows (RP x 16 pixels x CT channels fp32, pixel pitch
//      CT*4 + 16 bytes: conflict-free 16-byte writes) and a lane then owns 8 consecutive channels of a pixel: item i of a pass =
//      pixel (i * 256 + tid) / (CT / 8) of the pass, channel group tid % (CT / 8); residual and output move as 16-byte pieces, 8 (or
//      16) lanes per pixel line.  RP = 8: two (four) passes inside the K loop's LDS; RP = 16 (wide64): one pass ----------------------
template <int CT, int BH, int RP> struct C3Lines {
  static constexpr int NPASS = BH / RP, CG = CT / 8, IPP = RP * 16 * CG / 256;    // passes, channel groups, items per thread and pass
  static constexpr int TPITCH = CT * 4 + 16, LDS_BYTES = RP * 16 * TPITCH;
  static_assert(256 % CG == 0, "a thread keeps its channel group from item to item");
  const int tid, cb, oy0, ox0, n;                                    // cb: the thread's first channel
  __device__ __forceinline__ C3Lines(const C3Tile& T, int tid_) : tid(tid_), cb(T.ct * CT + 8 * (tid_ % CG)), oy0(BH * T.by), ox0(16 * T.bx), n(T.n) {}
  // pixel of the pass (row-major, 16 columns): (i * 256 + tid) / CG, written so that hipcc sees a per-thread base plus a constant per item
  __device__ __forceinline__ int pixel(int i) const { return i * (256 / CG) + tid / CG; }
  // byte offset of item i's 8 channels in a tensor of channel stride cs (out of range outside the image)
  __device__ __forceinline__ unsigned offset(const C3Args& p, int pass, int i, int cs) const {
    const int pl = pixel(i), oy = oy0 + pass * RP + (pl >> 4), ox = ox0 + (pl & 15);
    return (oy < p.H && ox < p.W) ? ((unsigned)((n * p.H + oy) * p.W + ox) * (unsigned)cs + (unsigned)cb) * 2u : kOob;
  }
  __device__ __forceinline__ u32x4 res_load(const C3Args& p, __amdgpu_buffer_rsrc_t rsr, int pass, int i) const {
    return __builtin_amdgcn_raw_buffer_load_b128(rsr, offset(p, pass, i, p.res_cs), 0, 0);
  }
};

// 8 channels of a pixel: folded BN, residual, ReLU, one 16-byte bf16x8 store
__device__ __forceinline__ void c3_finish8(const C3Args& p, __amdgpu_buffer_rsrc_t rsy, const f32x4 (&a)[2], const f32x4 (&sc)[2],
                                           const f32x4 (&sh)[2], u32x4 res, unsigned yo) {
  float o[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) { o[j] = fmaf(a[0][j], sc[0][j], sh[0][j]); o[4 + j] = fmaf(a[1][j], sc[1][j], sh[1][j]); }
  if (p.res) {
    const bf16x8 r8 = __builtin_bit_cast(bf16x8, res);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] += (float)r8[j];
  }
  if (p.relu) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = fmaxf(o[j], 0.f);
  }
  bf16x8 ob;
#pragma unroll
  for (int j = 0; j < 8; ++j) ob[j] = (__bf16)o[j];
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ob), rsy, yo, 0, 0);
}

// the epilogue of a tile whose K loop is over.  RES_EARLY: the residual is already in rv[NPASS * IPP] (requested in the prologue);
// else each pass requests its own, in flight under the transpose
template <int CT, int BH, int RP, bool RES_EARLY, int MT, int NRV>
__device__ __forceinline__ void c3_line_epilogue(const C3Args& p, const C3Tile& T, char* lds, const f32x4 (&acc)[4][MT], const u32x4 (&rv)[NRV],
                                                 __amdgpu_buffer_rsrc_t rsy, __amdgpu_buffer_rsrc_t rsr, int tid, int wm, int wn) {
  using L = C3Lines<CT, BH, RP>;
  static_assert(!RES_EARLY || NRV == L::NPASS * L::IPP, "one residual piece per item");
  const L ln(T, tid);
  const int col = tid & 15, kgl = (tid & 63) >> 4;
  c3_drain();                                                        // the look-ahead's last (zero-fill) DMAs still target LDS: drain before reuse
  // folded BN of the thread's 8 channels: the same for all its items, loaded once per tile (below)
  f32x4 sc[2] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 1.f, 1.f, 1.f}}, sh[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int pass = 0; pass < L::NPASS; ++pass) {
    u32x4 rq[L::IPP];
    if constexpr (!RES_EARLY) {
      if (p.res) {
#pragma unroll
        for (int i = 0; i < L::IPP; ++i) rq[i] = ln.res_load(p, rsr, pass, i);
      }
    }
    if (pass) __syncthreads();                                       // the previous pass's reads are done
    // this wave's rows lie in the pass (wave-uniform).  One pass holds every wave's rows, which hipcc cannot see from `wm` (a
    // readfirstlane): without the compile-time operand wide64 gets a scalar branch here and 14 more VGPRs
    if (L::NPASS == 1 || (wm * MT) / RP == pass) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          *reinterpret_cast<f32x4*>(lds + (((wm * MT + mt) - pass * RP) * 16 + col) * L::TPITCH + (wn * 64 + nt * 16 + 4 * kgl) * 4) = acc[nt][mt];
    }
    __syncthreads();
    if (pass == 0) {                                                 // (not earlier: requested ahead of the transpose they lengthen the accumulators'
                                                                     //  live ranges and hipcc stops updating wide64's accumulators in place in its K loop)
      if (p.scale) { sc[0] = *reinterpret_cast<const f32x4*>(p.scale + ln.cb); sc[1] = *reinterpret_cast<const f32x4*>(p.scale + ln.cb + 4); }
      if (p.shift) { sh[0] = *reinterpret_cast<const f32x4*>(p.shift + ln.cb); sh[1] = *reinterpret_cast<const f32x4*>(p.shift + ln.cb + 4); }
    }
#pragma unroll
    for (int i = 0; i < L::IPP; ++i) {
      const char* tp = lds + ln.pixel(i) * L::TPITCH + (tid % L::CG) * 32;
      const f32x4 a[2] = {*reinterpret_cast<const f32x4*>(tp), *reinterpret_cast<const f32x4*>(tp + 16)};
      u32x4 r;
      if constexpr (RES_EARLY) r = rv[pass * L::IPP + i]; else r = rq[i];
      c3_finish8(p, rsy, a, sc, sh, r, ln.offset(p, pass, i, p.y_cs));
    }
  }
}

template <int CT, int PB, int BH>
__global__ __launch_bounds__(256, (C3Geo<CT, PB, BH>::WG_PER_CU)) void conv3x3_bf16(const C3Args p) {
  using Geo = C3Geo<CT, PB, BH>;
  constexpr int PATCH_BYTES = Geo::PATCH_BYTES, PIXB = Geo::PIXB, ROWB = Geo::ROWB, PH = Geo::PH, PPW = Geo::PPW, FPW = Geo::FPW;
  constexpr int WN = Geo::WN, MT = Geo::MT, NT = Geo::NT, WSTEP = Geo::WSTEP, RB = Geo::RB, D = RB - 1;
  using Lines = C3Lines<CT, BH, 8>;
  static_assert(Lines::LDS_BYTES <= Geo::LDS_BYTES, "transpose tile does not fit the kernel's LDS");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* const patch = lds;                                // [PB][PATCH_BYTES]
  char* const ring = lds + PB * PATCH_BYTES;              // [RB][WSTEP]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int NCH = p.Cin >> 5, S = 9 * NCH;
  const C3Tile T = c3_decode(p, xcd_remap(blockIdx.x, gridDim.x));   // XCD-contiguous
  const __amdgpu_buffer_rsrc_t rsx = c3_rsrc(p.x, kOob), rsw = c3_rsrc(p.wp, p.wbytes), rsy = c3_rsrc(p.y, kOob), rsr = c3_rsrc(p.res, kOob);
  const unsigned w_tile = (unsigned)(T.ct * S) * (unsigned)WSTEP;
  int xa[3][2];
  c3_frag_addrs<PIXB>(xa, wm * MT, lane);
  const char* const wfrag = ring + wn * 4096 + lane * 16;             // + slot * WSTEP + nt * 1024
  u32x4 rv[Geo::RES_EARLY ? Lines::NPASS * Lines::IPP : 1];           // the 64-channel / two-buffer variant requests its residual in the prologue

  int mt_live = p.H - (BH * T.by + wm * MT);                          // pixel rows of this wave inside the image (wave-uniform)
  mt_live = mt_live < 0 ? 0 : (mt_live > MT ? MT : mt_live);
  f32x4 acc[NT][MT];
  c3_zero(acc);

  // (diagnostic only: p.stamps is null in every product launch; the stamps go to a buffer nothing else reads)
  auto stamp = [&](int i) {
    if (p.stamps && tid == 0) p.stamps[(size_t)blockIdx.x * 4 + i] = __builtin_amdgcn_s_memtime();
  };
  stamp(0);
  // ---- prologue: filters of steps 0 .. D-1, patch chunk 0 (and the residual: one HBM round trip covers both) ----------------
#pragma unroll
  for (int s = 0; s < D; ++s) c3_ring_dma<FPW>(rsw, ring + s * WSTEP, wave, lane, w_tile + (unsigned)s * (unsigned)WSTEP);
  c3_patch_dma<PIXB, PH, 0, PPW, true>(p, rsx, T, patch, wave, lane, 0, true);
  if constexpr (Geo::RES_EARLY) {
    if (p.res) {
      const Lines ln(T, tid);
#pragma unroll
      for (int k = 0; k < Lines::NPASS * Lines::IPP; ++k) rv[k] = ln.res_load(p, rsr, k / Lines::IPP, k % Lines::IPP);
    }
  }
  c3_drain();
  stamp(1);

  // One step = one filter tap of one 32-channel chunk: MT x NT MFMAs per wave, under the filter DMA of step s + D and (two-buffer
  // variant, taps 0 .. PPW-1; zeros past the last chunk) one piece of the NEXT chunk's patch; the wait: c3_step_vmcnt.
  static_assert(PB == 1 || PPW <= 9, "one patch piece per tap");
  int slot = 0;                                                      // ring slot of the current step
  auto kloop = [&](auto lv) {                                        // lv: pixel rows of this wave that take part
    for (int c = 0; c < NCH; ++c) {
      const int pbuf = PB == 2 ? (c & 1) : 0, s0 = 9 * c;
      if (PB == 1 && c > 0) {                                        // every wave has left the previous chunk (barrier): refill in place
        c3_patch_dma<PIXB, PH, 0, PPW, true>(p, rsx, T, patch, wave, lane, (unsigned)(c * 64), true);
        c3_drain();
      }
      const unsigned psoff = (unsigned)((c + 1) * 64);               // next chunk: + 32 channels
      const bool pnext = c + 1 < NCH;
      c3_nine_taps([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        c3_ring_dma<FPW>(rsw, ring + c3_ring_ahead<RB>(slot) * WSTEP, wave, lane, w_tile + (unsigned)(s0 + t + D) * (unsigned)WSTEP);
        if constexpr (PB == 2 && t < PPW) c3_patch_dma<PIXB, PH, t, t + 1, true>(p, rsx, T, patch + (pbuf ^ 1) * PATCH_BYTES, wave, lane, psoff, pnext);
        c3_mma<t, decltype(lv)::value, ROWB>(acc, wfrag + slot * WSTEP, patch + pbuf * PATCH_BYTES, xa);
        slot = c3_ring_next<RB>(slot);
        c3_step_wait<c3_step_vmcnt(t, D, FPW, PPW, PB)>();
      });
    }
  };
  // Bottom-edge blocks: a wave's pixel rows below the image are skipped in quarters of its MT rows (wave-uniform choice of a loop
  // specialised at compile time; per-row branches inside one loop cost hipcc 245 spilled registers).  With two to four workgroups per
  // CU the matrix-pipe and LDS cycles those rows would have burnt go to the co-resident workgroups (H = 57: 7 of 64 rows, H = 113:
  // 15 of 128).  Skipped rows keep their zero accumulators and are never stored.
  constexpr int QM = MT / 4;
  switch ((mt_live + QM - 1) / QM) {
    case 0: kloop(std::integral_constant<int, 0>{}); break;
    case 1: kloop(std::integral_constant<int, QM>{}); break;
    case 2: kloop(std::integral_constant<int, 2 * QM>{}); break;
    case 3: kloop(std::integral_constant<int, 3 * QM>{}); break;
    default: kloop(std::integral_constant<int, MT>{}); break;
  }

  stamp(2);
  c3_line_epilogue<CT, BH, 8, Geo::RES_EARLY>(p, T, lds, acc, rv, rsy, rsr, tid, wm, wn);
  if (p.stamps) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // (diagnostic: the stores have been acknowledged)
    stamp(3);
  }
}

// ---- Cin = 64 (ResNet layer1): both 32-channel halves of the patch in ONE image, fetched as whole 128-byte lines ---------------------
// Hypothesis behind it: layer1 is bound by a throughput between L2 and the CU (3.1c); its patch DMA asks for 64 of every pixel's 128 bytes
// per chunk, i.e. 16 half-used cache lines per instruction, and the other halves a microsecond later.  Here a pixel's 128 bytes sit
// together in LDS ([pixel][2 halves][4 x 16 B], 46 KB, one buffer), every DMA piece is 8 pixels x 128 contiguous bytes, the whole patch is
// requested in the prologue and the K loop issues filter DMA only.  Price: 128-byte pixel pitch -> the x-fragment reads are 2-way bank
// conflicts (16 lanes over 8 distinct 16-byte slots of each 128-byte half-window).  Same arithmetic in the same order as the other variants.
// The line epilogue runs in one pass of 16 rows (the K loop's LDS holds it) with the residual requested in the prologue.
template <int CT>
__global__ __launch_bounds__(256, 2) void conv3x3_bf16_wide64(const C3Args p) {
  using Geo = C3GeoWide64;
  static_assert(CT == Geo::CT, "64 output channels per workgroup");
  constexpr int MT = Geo::MT, NT = Geo::NT, WSTEP = Geo::WSTEP, RB = Geo::RB, D = RB - 1, FPW = Geo::FPW;
  using Lines = C3Lines<CT, Geo::BH, 16>;
  static_assert(Lines::LDS_BYTES <= Geo::LDS_BYTES && Lines::NPASS == 1, "transpose tile does not fit the kernel's LDS");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* const patch = lds;
  char* const ring = lds + Geo::PATCH_BYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // = the wave's block of MT pixel rows
  const C3Tile T = c3_decode(p, xcd_remap(blockIdx.x, gridDim.x));
  const __amdgpu_buffer_rsrc_t rsx = c3_rsrc(p.x, kOob), rsw = c3_rsrc(p.wp, p.wbytes), rsy = c3_rsrc(p.y, kOob), rsr = c3_rsrc(p.res, kOob);
  const unsigned w_tile = (unsigned)(T.ct * Geo::S) * (unsigned)WSTEP;

  // ---- prologue: filters of steps 0 .. D-1, the whole patch, the residual ------------------------------------------------------------
#pragma unroll
  for (int s = 0; s < D; ++s) c3_ring_dma<FPW>(rsw, ring + s * WSTEP, wave, lane, w_tile + (unsigned)s * (unsigned)WSTEP);
  c3_patch_dma<Geo::PIXB, Geo::PH, 0, Geo::PPW, false>(p, rsx, T, patch, wave, lane, 0, true);
  int xa[3][2];
  c3_frag_addrs<Geo::PIXB>(xa, wave * MT, lane);
  const char* const wfrag = ring + lane * 16;
  const Lines ln(T, tid);
  u32x4 rv[Lines::IPP];
  if (p.res) {
#pragma unroll
    for (int i = 0; i < Lines::IPP; ++i) rv[i] = ln.res_load(p, rsr, 0, i);
  }
  f32x4 acc[NT][MT];
  c3_zero(acc);
  c3_drain();

  int slot = 0;
  for (int c = 0; c < 2; ++c) {                                      // the two channel halves of the image, 64 bytes apart in every pixel
    c3_nine_taps([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      c3_ring_dma<FPW>(rsw, ring + c3_ring_ahead<RB>(slot) * WSTEP, wave, lane, w_tile + (unsigned)(9 * c + t + D) * (unsigned)WSTEP);
      c3_mma<t, MT, Geo::ROWB>(acc, wfrag + slot * WSTEP, patch + c * 64, xa);
      slot = c3_ring_next<RB>(slot);
      c3_step_wait<c3_step_vmcnt(t, D, FPW, 0, 1)>();                // filter DMA only
    });
  }
  c3_line_epilogue<CT, Geo::BH, 16, true>(p, T, lds, acc, rv, rsy, rsr, tid, wave, 0);
}

// ---- persistent form (two patch buffers, 16-row blocks): a workgroup walks a list of tiles and the DMA schedule simply runs on ---------
// In-kernel stamps on layer1 (64 -> 64, K = 576): a tile has 4.6k cycles of MFMA work per wave and lives 29k -- 8.3k waiting for its first
// patch and residual (HBM), 15k in the K loop, 6k in the epilogue until its stores are acknowledged; occupancy (2-4 workgroups per CU) cannot
// cover that, and a bigger tile changes nothing.  Here the schedule of conv3x3_bf16 is not cut at the tile boundary: in a tile's LAST chunk
// the "next chunk" patch pieces are chunk 0 of the NEXT tile, the filter look-ahead runs on into the next tile's first steps, the residual is
// requested at the start of the last chunk (64-channel tiles) and the epilogue's stores drain under the next tile's first steps.  The waits
// stay exact counts: loads, DMAs and stores retire in order, so a wait may leave in flight whatever was issued after the filters it names --
// the residual loads in the last chunk's first D steps, the previous tile's stores in a tile's first D-1 steps.
// Each XCD owns a contiguous eighth of the tile list and its workgroups sweep it side by side (neighbouring tiles share halo rows in L2).
// Its epilogue is a different design from the line epilogue: straight from the accumulator registers, 4 channels (8 bytes) per lane and store.
template <int CT>
__global__ __launch_bounds__(256, 2) void conv3x3_bf16_persist(const C3Args p, const int ntiles) {
  using Geo = C3Geo<CT, 2, 16>;
  constexpr int PATCH_BYTES = Geo::PATCH_BYTES, PIXB = Geo::PIXB, ROWB = Geo::ROWB, PH = Geo::PH, PPW = Geo::PPW, FPW = Geo::FPW;
  constexpr int WN = Geo::WN, MT = Geo::MT, NT = Geo::NT, WSTEP = Geo::WSTEP, RB = Geo::RB, D = RB - 1;
  constexpr bool RES_LATE = CT == 64;                              // residual requested at the start of the last chunk (MT*NT loads per wave)
  constexpr int NRES = MT * NT, NST = MT * NT;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* const patch = lds;
  char* const ring = lds + 2 * PATCH_BYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int NCH = p.Cin >> 5, S = 9 * NCH;

  // ---- this workgroup's tiles: XCD x = blockIdx & 7 owns tiles [start, start + len); its gx workgroups take start + li, start + li + gx, ..
  const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
  const int gx = ((int)gridDim.x + 7 - xcd) >> 3;
  const int q8 = ntiles >> 3, r8 = ntiles & 7;
  const int t_end = xcd * q8 + (xcd < r8 ? xcd : r8) + q8 + (xcd < r8 ? 1 : 0);
  int tile = xcd * q8 + (xcd < r8 ? xcd : r8) + li;
  if (tile >= t_end) return;                                        // (workgroup-uniform; before any barrier)

  const __amdgpu_buffer_rsrc_t rsx = c3_rsrc(p.x, kOob), rsw = c3_rsrc(p.wp, p.wbytes), rsy = c3_rsrc(p.y, kOob), rsr = c3_rsrc(p.res, kOob);
  const int col = lane & 15, kgl = lane >> 4;
  int xa[3][2];
  c3_frag_addrs<PIXB>(xa, wm * MT, lane);
  const char* const wfrag = ring + wn * 4096 + lane * 16;

  // ---- prologue of the FIRST tile only: filters of its steps 0 .. D-1, patch chunk 0 ------------------------------------------------
  C3Tile cur = c3_decode(p, tile);
  int nxt_id = tile + gx;
  C3Tile nxt = c3_decode(p, nxt_id < t_end ? nxt_id : tile);
  bool has_next = nxt_id < t_end;
  const unsigned wslab = (unsigned)S * (unsigned)WSTEP;             // bytes of one channel tile's filters
  unsigned wofs = (unsigned)cur.ct * wslab;                         // look-ahead cursor: where the filters of step (current + D) are
  int ahead_left = S;                                               // steps left in the cursor's tile
#pragma unroll
  for (int s = 0; s < D; ++s) {
    c3_ring_dma<FPW>(rsw, ring + s * WSTEP, wave, lane, wofs);
    wofs += WSTEP;
  }
  ahead_left -= D;
  c3_patch_dma<PIXB, PH, 0, PPW, true>(p, rsx, cur, patch, wave, lane, 0, true);
  c3_drain();

  int slot = 0;
  int pbuf = 0;                                                     // patch buffer of the current chunk (runs on across tiles)
  f32x4 acc[NT][MT];
  u32x2 rv[RES_LATE ? MT : 1][NT];
  // per-tile output addressing
  int co0, ox, oy0;
  unsigned pixel0;
  auto out_ok = [&](int mt) { return ox < p.W && oy0 + mt < p.H; };
  auto load_res = [&](int mt, u32x2 (&dst)[NT]) {
    const unsigned ro = out_ok(mt) ? ((pixel0 + (unsigned)(mt * p.W)) * (unsigned)p.res_cs + (unsigned)co0) * 2u : kOob;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) dst[nt] = __builtin_amdgcn_raw_buffer_load_b64(rsr, ro, (unsigned)(nt * 32), 0);
  };

  // one step; AFTER = first chunk of a tile that follows an epilogue (its NST stores are still draining), LASTC = the tile's last chunk;
  // ptile / psoff / plive: the patch that streams in under the chunk.  (step, chunk and kloop stay three nested lambdas, with the row
  // count an argument although it is always MT: folded into one, hipcc lays the four chunk copies out in another order
  // than it always had)
  auto step = [&](auto tc, auto livec, auto afterc, auto lastc, const C3Tile& ptile, const unsigned psoff, const bool plive) {
    constexpr int t = decltype(tc)::value;
    constexpr bool AFTER = decltype(afterc)::value, LASTC = decltype(lastc)::value;
    c3_ring_dma<FPW>(rsw, ring + c3_ring_ahead<RB>(slot) * WSTEP, wave, lane, wofs);
    wofs += WSTEP;
    if (--ahead_left == 0) {                                      // the cursor enters the next tile (or runs off the list: zeros)
      wofs = has_next ? (unsigned)nxt.ct * wslab : p.wbytes;
      ahead_left = has_next ? S : (1 << 30);
    }
    if constexpr (t < PPW) c3_patch_dma<PIXB, PH, t, t + 1, true>(p, rsx, ptile, patch + (pbuf ^ 1) * PATCH_BYTES, wave, lane, psoff, plive);
    if constexpr (RES_LATE && LASTC && t == 0) {
      if (p.res) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) load_res(mt, rv[mt]);
      } else {                                                    // keep the queue's shape (the counts are compile-time)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) rv[mt][nt] = __builtin_amdgcn_raw_buffer_load_b64(rsr, kOob, 0, 0);
      }
    }
    c3_mma<t, decltype(livec)::value, ROWB>(acc, wfrag + slot * WSTEP, patch + pbuf * PATCH_BYTES, xa);
    slot = c3_ring_next<RB>(slot);
    c3_step_wait<c3_step_vmcnt(t, D, FPW, PPW, 2, RES_LATE && LASTC ? NRES : 0, AFTER ? NST : 0)>();
  };
  auto chunk = [&](auto lv, auto afterc, auto lastc, const C3Tile& ptile, const unsigned psoff, const bool plive) {
    c3_nine_taps([&](auto tc) { step(tc, lv, afterc, lastc, ptile, psoff, plive); });
    pbuf ^= 1;
  };
  using TT = std::true_type;
  using FF = std::false_type;
  bool first_tile = true;
  for (;;) {
    co0 = cur.ct * CT + wn * 64 + 4 * kgl;
    ox = 16 * cur.bx + col;
    oy0 = 16 * cur.by + wm * MT;
    pixel0 = (unsigned)((cur.n * p.H + oy0) * p.W + ox);
    c3_zero(acc);
    auto kloop = [&](auto lv) {
      for (int c = 0; c < NCH; ++c) {
        const bool lastc = c + 1 == NCH, after = c == 0 && !first_tile;
        // the patch that streams in under this chunk: the next chunk of this tile, or chunk 0 of the next tile
        const C3Tile& ptile = lastc ? nxt : cur;
        const unsigned psoff = lastc ? 0u : (unsigned)((c + 1) * 64);
        const bool plive = lastc ? has_next : true;
        if (lastc) { if (after) chunk(lv, TT{}, TT{}, ptile, psoff, plive); else chunk(lv, FF{}, TT{}, ptile, psoff, plive); }
        else       { if (after) chunk(lv, TT{}, FF{}, ptile, psoff, plive); else chunk(lv, FF{}, FF{}, ptile, psoff, plive); }
      }
    };
    kloop(std::integral_constant<int, MT>{});                      // (no dead-row specialisation here: every extra copy of the loop cost registers)

    // ---- epilogue of this tile (its stores drain under the next tile's first steps) ----------------------------------------------
    f32x4 sc[NT], sh[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      sc[nt] = p.scale ? *reinterpret_cast<const f32x4*>(p.scale + co0 + nt * 16) : f32x4{1.f, 1.f, 1.f, 1.f};
      sh[nt] = p.shift ? *reinterpret_cast<const f32x4*>(p.shift + co0 + nt * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    constexpr int RD = RES_LATE ? 1 : 4;
    u32x2 rq[RD][NT];
    if constexpr (!RES_LATE) {
      if (p.res) {
#pragma unroll
        for (int mt = 0; mt < RD; ++mt) load_res(mt, rq[mt]);
      }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const unsigned yo = out_ok(mt) ? ((pixel0 + (unsigned)(mt * p.W)) * (unsigned)p.y_cs + (unsigned)co0) * 2u : kOob;
      u32x2 rr[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if constexpr (RES_LATE) rr[nt] = rv[mt][nt]; else rr[nt] = rq[mt % RD][nt];
      }
      if constexpr (!RES_LATE) {
        if (p.res && mt + RD < MT) load_res(mt + RD, rq[mt % RD]);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(acc[nt][mt][j], sc[nt][j], sh[nt][j]);
        if (p.res) {
          const bf16x4 r4 = __builtin_bit_cast(bf16x4, rr[nt]);
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] += (float)r4[j];
        }
        if (p.relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
        }
        bf16x4 ob;
#pragma unroll
        for (int j = 0; j < 4; ++j) ob[j] = (__bf16)o[j];
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, ob), rsy, yo, (unsigned)(nt * 32), 0);
      }
    }
    if (!has_next) break;
    first_tile = false;
    tile = nxt_id;
    cur = nxt;
    nxt_id = tile + gx;
    has_next = nxt_id < t_end;
    nxt = c3_decode(p, has_next ? nxt_id : tile);
  }
}

// OHWI bf16 filters [Cout][3][3][Cin] -> [ct][chunk][tap][CT/16][lane][8]: element j of lane (m = lane & 15, kg = lane >> 4)
// of fragment nt is w[ct*CT + nt*16 + m][tap][chunk*32 + kg*8 + j]
__global__ __launch_bounds__(256) void conv3x3_pack(const unsigned short* __restrict__ w, unsigned short* __restrict__ out, int Cout,
                                                    int Cin, int CT, long long total) {
  const long long idx = blockIdx.x * 256ll + threadIdx.x;            // one 16-byte fragment piece each
  if (idx >= total) return;
  const int NCH = Cin >> 5, nfr = CT / 16;
  long long r = idx;
  const int lane = (int)(r & 63); r >>= 6;
  const int nt = (int)(r % nfr); r /= nfr;
  const int tap = (int)(r % 9); r /= 9;
  const int c = (int)(r % NCH);
  const int ct = (int)(r / NCH);
  const int co = ct * CT + nt * 16 + (lane & 15), ci = c * 32 + (lane >> 4) * 8;
  typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
  u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (co < Cout) v = *reinterpret_cast<const u16x8*>(w + ((size_t)co * 9 + tap) * Cin + ci);
  *reinterpret_cast<u16x8*>(out + idx * 8) = v;
}

}  // namespace

// Output-channel tile the kernel will use for a layer (the packed filter image depends on it).
extern "C" int bevf_conv3x3_bf16_ct(int Cout) { return Cout % 128 == 0 ? 128 : 64; }

extern "C" size_t bevf_conv3x3_pack_elems(int Cout, int Cin) {
  const int CT = bevf_conv3x3_bf16_ct(Cout);
  return (size_t)((Cout + CT - 1) / CT) * CT * 9 * (size_t)Cin;
}

extern "C" int bevf_conv3x3_pack_bf16(const void* w_ohwi, void* packed, int Cout, int Cin, void* stream) {
  BEVF_REQUIRE(w_ohwi && packed, "conv3x3_pack: null pointer");
  BEVF_REQUIRE(Cout > 0 && Cin > 0 && Cin % 32 == 0, "conv3x3_pack: Cin=%d must be a positive multiple of 32", Cin);
  BEVF_REQUIRE(bevf_aligned16(w_ohwi) && bevf_aligned16(packed), "conv3x3_pack: pointers must be 16-byte aligned");
  const int CT = bevf_conv3x3_bf16_ct(Cout);
  const long long total = (long long)bevf_conv3x3_pack_elems(Cout, Cin) / 8;
  hipLaunchKernelGGL(conv3x3_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(w_ohwi), static_cast<unsigned short*>(packed), Cout, Cin, CT, total);
  return bevf_check_launch("bevf_conv3x3_pack_bf16");
}

static unsigned long long* g_c3_stamps = nullptr;
// Diagnostic (tools/conv3x3_bench.py stamps): buf = device buffer of 4 x 8 bytes per workgroup of the NEXT launches, or null to stop
extern "C" int bevf_debug_conv3x3_stamps(void* buf) {
  g_c3_stamps = static_cast<unsigned long long*>(buf);
  return BEVF_OK;
}

extern "C" int bevf_conv3x3_bf16(const bevf_conv_desc* d, void* stream) {
  BEVF_REQUIRE(d && d->x && d->w && d->y, "conv3x3_bf16: null x / w / y");
  BEVF_REQUIRE(d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1, "conv3x3_bf16: 3x3, stride 1, pad 1 only (got %dx%d s%d p%d)",
               d->KH, d->KW, d->stride, d->pad);
  BEVF_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cout > 0 && d->Ho == d->H && d->Wo == d->W, "conv3x3_bf16: bad shape");
  BEVF_REQUIRE(d->Cin > 0 && d->Cin % 32 == 0, "conv3x3_bf16: Cin=%d must be a positive multiple of 32", d->Cin);
  BEVF_REQUIRE(d->Cout % 64 == 0, "conv3x3_bf16: Cout=%d must be a multiple of 64", d->Cout);
  BEVF_REQUIRE(d->x_cs >= d->Cin && d->x_cs % 8 == 0, "conv3x3_bf16: x_cs=%d must be >= Cin and a multiple of 8", d->x_cs);
  BEVF_REQUIRE(d->y_cs >= d->Cout && d->y_cs % 4 == 0, "conv3x3_bf16: y_cs=%d must be >= Cout and a multiple of 4", d->y_cs);
  BEVF_REQUIRE(!d->res || (d->res_cs >= d->Cout && d->res_cs % 4 == 0), "conv3x3_bf16: res_cs must be >= Cout and a multiple of 4");
  BEVF_REQUIRE(!d->colmax && !d->stats && !d->bnb_x, "conv3x3_bf16: no column max / BatchNorm epilogues (inference kernel)");
  BEVF_REQUIRE(bevf_aligned16(d->x) && bevf_aligned16(d->w) && (reinterpret_cast<uintptr_t>(d->y) & 7u) == 0 &&
                   (!d->res || (reinterpret_cast<uintptr_t>(d->res) & 7u) == 0) &&
                   (!d->scale || bevf_aligned16(d->scale)) && (!d->shift || bevf_aligned16(d->shift)),
               "conv3x3_bf16: x / w / scale / shift must be 16-byte aligned, y / res 8-byte aligned");
  BEVF_REQUIRE((long long)d->N * d->H * d->W * d->x_cs * 2 < (1ll << 31) && (long long)d->N * d->H * d->W * d->y_cs * 2 < (1ll << 31) &&
                   (!d->res || (long long)d->N * d->H * d->W * d->res_cs * 2 < (1ll << 31)),
               "conv3x3_bf16: activations must stay below 2 GiB (32-bit buffer offsets)");
  const size_t wbytes = bevf_conv3x3_pack_elems(d->Cout, d->Cin) * 2;
  BEVF_REQUIRE(wbytes < (1ull << 31), "conv3x3_bf16: packed filters must stay below 2 GiB");
  const int CT = bevf_conv3x3_bf16_ct(d->Cout);
  // tile: 0 = auto (tools/conv3x3_bench.py); 64-channel tiles only: 1 = two patch buffers (2 workgroups per CU), 2 = one (4 per CU),
  // 3 = one buffer and 32-row blocks (2 per CU), 4 = persistent, 5 = both channel halves in one patch image (Cin = 64)
  const bool wide64 = CT == 64 && d->Cin == 64 && (d->tile == 5 || (d->tile == 0 && C3_AUTO_WIDE64));
  const bool persist = !wide64 && CT == 64 && (d->tile == 4 || (d->tile == 0 && C3_AUTO_PERSIST && d->Cin < 128));
  const int variant = CT == 128 ? 1 : ((d->tile && d->tile < 4) ? d->tile : (d->Cin >= 128 ? 2 : C3_AUTO_SHORTK));
  const int BH = (!wide64 && !persist && variant == 3) ? 32 : 16;    // block height of the kernel chosen
  C3Args a{};
  a.x = d->x; a.wp = d->w; a.scale = d->scale; a.shift = d->shift; a.res = d->res; a.y = d->y;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.x_cs = d->x_cs; a.y_cs = d->y_cs; a.res_cs = d->res_cs;
  a.relu = d->relu;
  a.TBY = (d->H + BH - 1) / BH; a.TBX = (d->W + 15) / 16;
  a.wbytes = (unsigned)wbytes;
  a.stamps = g_c3_stamps;
  const long long ntiles = (long long)d->N * a.TBY * a.TBX * (d->Cout / CT);
  BEVF_REQUIRE(ntiles < (1ll << 31), "conv3x3_bf16: too many tiles");
  const dim3 grid((unsigned)ntiles), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const char* const entry = "bevf_conv3x3_bf16";
  if (wide64) return bevf_launch(entry, conv3x3_bf16_wide64<64>, grid, block, C3GeoWide64::LDS_BYTES, st, a);
  if (persist) {
    const dim3 pgrid((unsigned)(ntiles < 512 ? ntiles : 512));      // 2 workgroups per CU
    return bevf_launch(entry, conv3x3_bf16_persist<64>, pgrid, block, C3Geo<64, 2, 16>::LDS_BYTES, st, a, (int)ntiles);
  }
  if (CT == 128) return bevf_launch(entry, conv3x3_bf16<128, 2, 16>, grid, block, C3Geo<128, 2, 16>::LDS_BYTES, st, a);
  if (variant == 3) return bevf_launch(entry, conv3x3_bf16<64, 1, 32>, grid, block, C3Geo<64, 1, 32>::LDS_BYTES, st, a);
  if (variant == 2) return bevf_launch(entry, conv3x3_bf16<64, 1, 16>, grid, block, C3Geo<64, 1, 16>::LDS_BYTES, st, a);
  return bevf_launch(entry, conv3x3_bf16<64, 2, 16>, grid, block, C3Geo<64, 2, 16>::LDS_BYTES, st, a);
}
