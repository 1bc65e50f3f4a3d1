// fp32 Winograd F(2x2,3x3) convolution (3x3, stride 1, pad 1) on v_mfma_f32_16x16x4_f32, gfx950 -- fully fused:
// input transform in registers from a raw LDS patch, the 16 "frequency" GEMMs on the matrix pipe, output transform
// in registers, the same fused epilogue as conv_igemm (folded BN scale/shift, residual, ReLU, channel-strided store).
//
//   Y = A^T [ (G g G^T) .* (B^T d B) ] A      per 2x2 output tile, summed over input channels
//
// 16 multiplies per 4 outputs instead of 36: 2.25x fewer MFMA FLOPs than the implicit GEMM, and the fp32 MFMA pipe is
// what bounds these layers.  The products are fp32 FMAs with fp32 accumulation like the direct kernel;
// what changes is the summation structure, so results agree with it to a few 1e-7 relative, not bit for bit.
//
// Workgroup = 256 threads = 4 waves = 8x8 Winograd tiles (16x16 output pixels) x 64 output channels.  Wave w owns
// tile rows 2w, 2w+1 (16 tiles) x 64 channels x all 16 frequencies: 64 accumulator tiles of 16x16 = all 256 AGPRs
// (one wave per SIMD).  K loop over groups of 8 input channels = 2 MFMA k-steps of 128 MFMAs:
//   * A side: the 18x18-pixel input patch sits in LDS as raw NHWC rows (32-channel chunks, double-buffered, staged
//     global -> registers -> LDS with out-of-range pixels answered by the buffer unit with zeros); lane (t = l&15,
//     kq = l>>4) reads its tile's 4x4 patch for channels 2kq, 2kq+1 (16 ds_read_b64) and transforms it (64 VALU)
//     into the A fragments of all 16 frequencies, one group ahead of their use;
//   * B side: the transformed filters are stored in HBM in the exact LDS image order per (64-channel slab, group),
//     so staging is a straight 32 KB LDS-DMA copy (global_load_lds), double-buffered; fragments are ds_read_b128,
//     bank-conflict-free.
// With one wave per SIMD nothing else fills an issue gap, so every non-MFMA instruction is pinned BETWEEN two MFMAs
// (one small piece per gap, sched_barrier after each) and issues in the shadow of the MFMA executing.  The MFMAs are
// inline asm that names its accumulator registers literally (wino_common.h: mfma_named; accumulator (f, nb) = a[16 f + 4 nb ..
// + 3]) and the epilogue fetches each value with an asm v_accvgpr_read: hipcc is given no accumulator variable.  With the
// builtin its allocator moved accumulators between AGPRs and VGPRs inside the loop (44-296 v_accvgpr moves per group); as "+a"
// asm operands the loop was clean, but a tile loop around it spilled and shuffled them.
//
// RUNON (plain inference launches, Cin >= 64): one workgroup per CU walks the linear tiles b, b + G, b + 2G, ... and its K loop
// runs on into the next tile -- the staging slots that are idle in a tile's last groups fetch the next tile's first patch chunk
// and filter image, so only the epilogue and the slot offsets of the tile after next stand between two tiles' MFMAs.
#include "wino_common.h"

#include <map>
#include <mutex>

namespace {

struct WinoArgs {
  const float* x;      // NHWC, channel stride x_cs
  const float* u;      // [ct][G][16 f][2 nb pair][4 kq][16 n][2 nb][2 cin]: bevf_wino_filter_transform_f32
  const float* scale;  // [Cout] or null
  const float* shift;
  const float* res;    // NHWC residual or null
  float* y;
  float* stats;        // STATS: [nsp * 4][Cout][2] partial sums of (y - pivot), (y - pivot)^2;  BNB: of dy, dy * xhat
  const float* pivot;  // [Cout] or null
  // BNB (training backward): this conv's output is the gradient dY of a train-mode BatchNorm(+ReLU) layer; the epilogue applies
  // that layer's ReLU mask and leaves its backward sums (csrc/norm_train.hip: bn_bwd_partials) -- the layer's own raw
  // input bnb_x [pixels][Cout], its output bnb_y (mask source when the layer had a residual; else the mask is recomputed
  // from bnb_x with bn_apply's fma), and its per-channel mean / invstd / gamma / beta
  const float *bnb_x, *bnb_y, *bnb_mean, *bnb_invstd, *bnb_gamma, *bnb_beta;
  int N, H, W, Cin, x_cs, Cout, y_cs, res_cs;
  int TBY, TBX, nct;   // tile blocks per image (rows, cols), 64-channel slabs
  // Stacked rows (HS > 0): the N images are treated as ONE map of N * HS rows -- image n at rows n*HS .. n*HS+H-1, the HS - H rows
  // between two images dead (they read as zeros: they ARE the padding row both neighbours need) -- cut into SB block rows that
  // ignore image boundaries.  A 57-row map then wastes 1 row in 58 instead of 7 in 64.  HS is even (a tile's 2x2 alignment inside
  // its image, and with it every rounding, is what it is in the per-image tiling: the two are bit-identical) and > block height
  // (a patch spans at most two images).  HS = 0: block rows per image, SB = N * TBY.
  int HS, SB;
  unsigned div_mul;    // ceil(2^32 / HS) (stacked) or ceil(2^32 / TBY) (0 for TBY = 1): row -> image by one s_mul_hi (the host checks the range)
  // RUNON: linear tile L = (ct * nsp + sp) * ... -> ct = L / nsp, sp = rem / TBX, bx = rem % TBX, by multiply-high (ceil(2^32 / d), 0 for
  // d = 1; the host checks the range); the grid is (workgroups, 1, 1)
  int ntiles, nsp;
  unsigned nsp_mul, tbx_mul;
  unsigned long long* stamps;   // DIAG instantiations only (bevf_debug_wino_stamps): kWinoStamps x s_memtime per workgroup
};

constexpr int kWinoStamps = 6;  // start / first patch DMA issued / first operands transformed / K loop done / epilogue issued / stores acknowledged

constexpr int PITCH = 36;                                      // floats per patch pixel in LDS (32 + 4 pad); 18x18 or 34x10 pixels
constexpr int PDMA = 12;                                       // LDS-DMA instructions per wave and chunk (4 waves x 12 x 64 slots)
constexpr int PATCH_FLOATS = 4 * PDMA * 64 * 4;                // 12288 floats = 48 KiB: 9 16-byte slots per pixel (8 data + 1 pad), 2916 / 3060 slots rounded up to 48 x 64
constexpr int BG_FLOATS = 16 * 4 * 16 * 8;                     // 8192 floats = 32 KB per channel group
constexpr int LDS_BYTES = (2 * PATCH_FLOATS + 2 * BG_FLOATS) * 4;

// GEO = block geometry: 0 = 8x8 tiles (16x16 pixels; wave w: tile rows 2w, 2w+1), 1 = 16x4 tiles (32 rows x 8 columns; wave w:
// tile rows 4w .. 4w+3) -- the host takes whichever covers the map with fewer blocks (57x100: 28 -> 26, 113x200: 104 -> 100).
template <bool RES, bool RELU, bool STATS = false, int BNB = 0, int GEO = 0, bool DIAG = false, bool RUNON = false>
__global__ __launch_bounds__(256, 1) void wino_f32(const WinoArgs p) {
  static_assert(!RUNON || (!STATS && BNB == 0 && !DIAG), "the run-on tile loop has no barrier after a tile: plain epilogues only");
  auto stamp_at = [&](int i, unsigned long long tm) {                // diagnostic launches only; the buffer is read by nothing else
    if constexpr (DIAG) {
      if (threadIdx.x == 0) p.stamps[(size_t)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kWinoStamps + i] = tm;
    }
  };
  auto stamp = [&](int i) {
    if constexpr (DIAG) stamp_at(i, __builtin_amdgcn_s_memtime());
  };
  // (stamp 0 is taken here and stored with stamp 1: a store up here is a divergent branch that uses the workgroup ids, across which
  //  hipcc carried them in VGPRs -- every filter DMA of the K loop, whose scalar offset comes from ct, then ran in a v_readfirstlane loop)
  unsigned long long t_start = 0;
  if constexpr (DIAG) t_start = __builtin_amdgcn_s_memtime();
  constexpr int BHP = GEO ? 32 : 16, BWP = GEO ? 8 : 16;          // block height / width in pixels
  constexpr int PWP = BWP + 2, PIXG = (BHP + 2) * PWP;            // patch width, patch pixels (324 or 340)
  constexpr int PSLOTSG = PIXG * 9;
  static_assert(PSLOTSG <= 4 * PDMA * 64, "patch does not fit the DMA image");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const patch = lds;                                     // [2][patch pixels][PITCH] (padded to PATCH_FLOATS)
  float* const bbuf = lds + 2 * PATCH_FLOATS;                   // [2][BG_FLOATS]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = p.Cin >> 3;                                     // channel groups of 8
  const int NCH = p.Cin >> 5;                                   // patch chunks of 32 channels
  // grid = (TBX, SB, nct): dispatch order x, y, z = spatial blocks of one 64-channel slab first, so concurrent workgroups share one slab
  // of transformed filters (L2-resident); no index arithmetic to decode a tile.  RUNON: the same order as a linear tile index
  auto tile_of = [&](int lt, int& bx, int& sp, int& ct) {           // wave-uniform: scalar multiplies
    ct = p.nsp_mul ? (int)__umulhi((unsigned)lt, p.nsp_mul) : lt;
    const int rem = lt - ct * p.nsp;
    sp = p.tbx_mul ? (int)__umulhi((unsigned)rem, p.tbx_mul) : rem;
    bx = rem - sp * p.TBX;
  };
  // ---- patch staging by LDS-DMA (buffer_load ... lds: an out-of-range lane writes zeros -- the pad ring, the pad slot of
  //      every pixel, the slots past the patch): instruction (4 j + wave), j < 12, fills 64 consecutive 16-byte slots;
  //      slot s = pixel s / 9, piece s % 9 (8 = pad) --------------------------------------------------------------------
  const __amdgpu_buffer_rsrc_t rsx = buf_rsrc(p.x);
  // n / rb: image and in-image row of the block's first pixel row; hw: rows after which a row index wraps into the next image
  // The 12 slot offsets of a wave are what stands between the workgroup's start and its last HBM request (one wave per SIMD: ~5 cycles
  // per dependent instruction, ~2.5 k cycles in all -- as much as the wait that follows, tools/wino_stamps.py): 24-bit multiplies (every
  // factor is < 2^24: a pixel index because the tensor stays below 2 GiB with >= 32 channels of 4 bytes), no division (3D grid, one
  // s_mul_hi for the image of a row).
  // block row sp of the grid -> n0 / r0: image and in-image row of the patch's first row (block row - 1); n, rb, hw as above
  auto block_rows = [&](int sp, int& n0, int& r0, int& n, int& rb, int& hw) {
    if (p.HS) {
      const int s0 = BHP * sp - 1 + p.HS, q0 = (int)__umulhi((unsigned)s0, p.div_mul);   // s0 / HS (+ HS: the division never sees -1)
      n0 = q0 - 1;
      r0 = s0 - q0 * p.HS;
      hw = p.HS;
      const bool top = r0 + 1 == p.HS;                              // the patch's first row is the last (dead) row of image n0
      n = top ? q0 : n0;
      rb = top ? 0 : r0 + 1;
    } else {
      n0 = p.div_mul ? (int)__umulhi((unsigned)sp, p.div_mul) : sp;   // sp / TBY (TBY = 1: the multiplier 2^32 is passed as 0)
      rb = BHP * (sp - n0 * p.TBY);
      r0 = rb - 1;
      hw = 0x7fffffff;
      n = n0;
    }
  };
  // stacked rows: a row index at or past hw lies in the NEXT image -- made in-image here; -> whether it wrapped.  Whoever wraps then tests
  // image < N, row < H, column < W in its own terms
  auto wrap_row = [](int& row, int hw) {
    const bool wr = row >= hw;
    row -= wr ? hw : 0;
    return wr;
  };
  // byte offset in x of pixel pix (< 1024) of the patch that starts at row r0 of image n0, column ix0; ok: the pixel exists (inside the
  // image, not in a dead row, image < N) -- whoever uses the offset sends every other lane to kOob
  auto pixel_off = [&](unsigned pix, int n0, int r0, int hw, int ix0, bool& ok) {
    const unsigned py = __umul24(pix, GEO ? 6554u : 3641u) >> 16, px = pix - __umul24(py, (unsigned)PWP);   // pix / 10 (or / 18) for pix < 1024
    int iy = r0 + (int)py;
    const int ix = ix0 + (int)px;
    const bool wr = wrap_row(iy, hw);
    ok = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W && (unsigned)(n0 + (wr ? 1 : 0)) < (unsigned)p.N;
    const unsigned row = (unsigned)(n0 * p.H) + (wr ? (unsigned)p.H : 0u) + (unsigned)iy;       // image row index over the batch
    return __umul24(__umul24(row, (unsigned)p.W) + (unsigned)ix, (unsigned)(p.x_cs * 4));
  };
  auto patch_dma_from = [&](__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, int buf, int j) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(patch + buf * PATCH_FLOATS + (4 * j + wave) * 256),
                                             16, voff, soff, 0, 0);
  };
  auto patch_dma = [&](unsigned voff, unsigned soff, int buf, int j) { patch_dma_from(rsx, voff, soff, buf, j); };
  // the twelve slot offsets of this block's patch; each slot's chunk-0 DMA is issued as soon as its offset exists, so that its latency
  // and its transfer into LDS (48 KB at 64 bytes per clock: ~770 cycles for the patch) run under the arithmetic of the slots behind it
  // (issuec false: the offsets only -- a later tile's, whose DMAs the K loop issues)
  auto make_pv = [&](unsigned (&pv)[PDMA], auto issuec, int bx, int sp, int& n, int& rb, int& hw) {
    int n0, r0;
    block_rows(sp, n0, r0, n, rb, hw);
    const int ix0 = BWP * bx - 1;
#pragma unroll
    for (int j = 0; j < PDMA; ++j) {
      const unsigned sl = (unsigned)((4 * j + wave) * 64 + lane);
      const unsigned pix = __umul24(sl, 7282u) >> 16, piece = sl - 9u * pix;                    // sl / 9 for sl < 3072
      bool pok;
      const unsigned off = pixel_off(pix, n0, r0, hw, ix0, pok);
      const bool in_patch = (4 * j + 3) * 64 + 63 < PSLOTSG || sl < (unsigned)PSLOTSG;          // (wave < 4: only the last instruction's slots can lie past the patch)
      pv[j] = (in_patch && piece < 8u && pok) ? off + 16u * piece : kOob;
      if constexpr (decltype(issuec)::value) {
        patch_dma(pv[j], 0, 0, j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // RES: in a tile's LAST chunk the "next chunk" slots have nothing to fetch; two of them (group 0's first two) then touch one 16-byte
  // piece of every 128-byte line of this wave's residual pixels -- the data lands in the idle patch buffer and is never read, but the
  // lines are in L2 when the epilogue asks for them ~3 groups later (the epilogue waited 4.7k cycles for HBM here: tools/wino_stamps.py)
  // RUNON: those slots fetch the next tile's patch; the lines are touched by two ordinary one-dword loads per lane (pfv: their offsets,
  // kOob outside a tile's last chunk) into registers nobody reads
  const __amdgpu_buffer_rsrc_t rsr_pf = buf_rsrc(RES ? p.res : p.x);
  bool pf_res = false;                                              // group 0's part of the patch comes through rsr_pf
  unsigned pfv[2] = {kOob, kOob};
  unsigned junk[2] = {0u, 0u};
  // byte offset in res of residual line s2 * 64 + lane of this wave (its 64 pixels x two 128-byte halves of their 64 channels), or kOob
  auto res_line = [&](int s2, int n, int rb, int hw, int bx, int ct) {
    const int line = s2 * 64 + lane, pw = line >> 1;
    const int prow = GEO ? (pw >> 3) : (pw >> 4), pcol = GEO ? (pw & 7) : (pw & 15);
    int ry = rb + (GEO ? 8 : 4) * wave + prow;
    const bool wr = wrap_row(ry, hw);
    const int rn = n + (wr ? 1 : 0), rx = BWP * bx + pcol;
    const bool ok = rn < p.N && ry < p.H && rx < p.W && ct * 64 + (line & 1) * 32 < p.Cout;
    return ok ? (unsigned)((((rn * p.H + ry) * p.W + rx) * p.res_cs + ct * 64 + (line & 1) * 32) * 4) : kOob;
  };

  // ---- B staging by LDS-DMA: group image = 32 pieces of 1 KiB; wave w issues pieces 8w .. 8w+7 ----------------------
  // (buffer form: the per-lane part of the address is one constant VGPR, the image / piece offset a scalar -- the global
  //  form cost a 64-bit vector add per piece, and the fp32 MFMA shares the vector ALU)
  const __amdgpu_buffer_rsrc_t rsu = buf_rsrc(p.u);
  const unsigned u_lane = (unsigned)((wave * 8 * 256 + lane * 4) * 4);
  auto dma_piece = [&](unsigned img, int buf, int i) {              // img: byte offset of the group image in p.u
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsu, (__attribute__((address_space(3))) void*)(bbuf + buf * BG_FLOATS + wave * 8 * 256 + i * 256),
                                             16, u_lane, img + i * 1024, 0, 0);
  };

  // ---- compute roles --------------------------------------------------------------------------------------------
  const int t = lane & 15, kq = lane >> 4;
  const int ty = GEO ? 4 * wave + (t >> 2) : 2 * wave + (t >> 3), tx = GEO ? (t & 3) : (t & 7);
  const int a_lane = ((2 * ty) * PWP + 2 * tx) * PITCH + 2 * kq;    // floats: patch pixel (2ty, 2tx), channels 2kq..
  const int b_lane = kq * 64 + t * 4;                              // floats within a [4 kq][16 n][2 nb][2 cin] block: lane * 16 bytes, linear

  // A fragments: two sets -- group g multiplies from set g & 1 while the WHOLE input transform of group g + 1 is written into the other
  // set in ONE MFMA gap: a lone VALU instruction between fp32 MFMAs costs ~15 cycles, the ones right behind it ~3 (probe),
  // so 32 packed adds cost ~120 cycles as one cluster and ~250 as the twelve they used to be
  f32x2 vv[2][16], dn[16];
  // columns c, c + 1 of row q of the 4x4 patch at pa -> dn[4q + c], dn[4q + c + 1]: 2 x ds_read_b64
  auto load_patch = [&](const float* pa, int q, int c) {
    dn[4 * q + c] = *reinterpret_cast<const f32x2*>(pa + (q * PWP + c) * PITCH);
    dn[4 * q + c + 1] = *reinterpret_cast<const f32x2*>(pa + (q * PWP + c + 1) * PITCH);
  };
  auto transform_into = [&](f32x2 (&v)[16]) {                       // B^T d B: dn (consumed) -> v
#pragma unroll
    for (int c = 0; c < 4; ++c) {                                   // B^T d, column c (in place)
      const f32x2 t0 = dn[0 + c] - dn[8 + c], t1 = dn[4 + c] + dn[8 + c], t2 = dn[8 + c] - dn[4 + c], t3 = dn[4 + c] - dn[12 + c];
      dn[0 + c] = t0; dn[4 + c] = t1; dn[8 + c] = t2; dn[12 + c] = t3;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                   // (B^T d) B, row r -> v[4r..4r+3]
      v[4 * r + 0] = dn[4 * r + 0] - dn[4 * r + 2];
      v[4 * r + 1] = dn[4 * r + 1] + dn[4 * r + 2];
      v[4 * r + 2] = dn[4 * r + 2] - dn[4 * r + 1];
      v[4 * r + 3] = dn[4 * r + 1] - dn[4 * r + 3];
    }
  };

  // ---- prologue: first tile's patch chunk 0, B group 0, A fragments of group 0 -----------------------------------------
  // pv: this tile's slot offsets; pvn (RUNON): the workgroup's next tile's (all kOob behind its last tile); pvl: what the staging slots
  // of the current chunk fetch
  unsigned pv[PDMA], pvn[PDMA], pvl[PDMA];
  int n, rb, hw, bx, ct, sp;
  int nn = 0, rbn = 0, hwn = 0, bxn = 0, ctn = 0;                   // RUNON: the next tile
  int lt = blockIdx.x;                                              // RUNON: this tile's linear index
  bool has_next = false;
  if constexpr (RUNON) {
    tile_of(lt, bx, sp, ct);
  } else {
    bx = blockIdx.x; sp = blockIdx.y; ct = blockIdx.z;
  }
  {                                                                 // filter DMA first: it flies while the slot offsets are computed
#pragma unroll
    for (int i = 0; i < 8; ++i) dma_piece((unsigned)(ct * G) * (BG_FLOATS * 4), 0, i);
  }
  make_pv(pv, std::true_type{}, bx, sp, n, rb, hw);
  // the offsets of the tile after this one: computed where nothing waits for them (the first tile's under its own first wait, later
  // ones between two tiles: the one serial piece the run-on loop keeps)
  auto make_next = [&]() {
    has_next = lt + (int)gridDim.x < p.ntiles;
    if (has_next) {
      int spn;
      tile_of(lt + (int)gridDim.x, bxn, spn, ctn);
      make_pv(pvn, std::false_type{}, bxn, spn, nn, rbn, hwn);
    } else {
#pragma unroll
      for (int j = 0; j < PDMA; ++j) pvn[j] = kOob;
    }
  };
  unsigned long long t_issued = 0;                                  // DIAG: everything the first wait depends on is in flight from here
  if constexpr (DIAG) t_issued = __builtin_amdgcn_s_memtime();
  // Staging schedule (filter image of group g+1 and a third of a later patch chunk per group, everything by LDS-DMA, no
  // register staging and no ds_write in the loop): chunk c+1's patch is fetched in three parts, in the last group of
  // chunk c-1 and groups 0, 1 of chunk c, always AFTER the group's filter pieces.  Loads retire in order, so the
  // hand-written wait at a group's end, vmcnt(4), names exactly the filter image and leaves the newest patch part in
  // flight: every patch load has at least a whole group (1.7 us) to land.  (A __syncthreads() waits vmcnt(0), and hipcc
  // adds vmcnt(0) before any ds_write that follows an LDS-DMA: in-kernel ablation put 13 % of the kernel on those waits.)
#pragma unroll
  for (int j = 0; j < 4; ++j) patch_dma(NCH > 1 ? pv[j] : kOob, 128, 1, j);
  if constexpr (RUNON) make_next();
  // (wait + barrier as ONE asm, as at a group's end: __syncthreads() waits vmcnt(0), i.e. also for the four chunk-1 loads just issued,
  //  which nothing reads before group 3; the first group's end, vmcnt(4) behind twelve younger loads, covers them)
  asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    load_patch(patch + a_lane, q, 0);
    load_patch(patch + a_lane, q, 2);
  }
  transform_into(vv[0]);
  int pbuf = 0;                                                     // patch buffer holding the current chunk
  stamp_at(0, t_start);
  stamp_at(1, t_issued);
  stamp(2);

  // one channel group (8 channels = 2 MFMA k-steps); gl = position in the 32-channel patch chunk (static)
  //   pvl / psoff: where the NEXT chunk's patch comes from; in the tile's last chunk the slots have nothing to fetch (kOob: the DMA
  //   writes zeros into the idle buffer) except, in the RES instantiations, group 0's first two: the residual prefetch (see rsr_pf)
  //   bimg: byte offset of the NEXT group's filter image in p.u (bnext false: nothing follows)
  auto group = [&](auto glc, auto firstc, const unsigned psoff, const unsigned bimg, const bool bnext) {
    constexpr int gl = decltype(glc)::value;
    constexpr bool kFirst = decltype(firstc)::value;      // a tile's first group: its k-step-0 MFMAs start the accumulators (C = 0)
    const int abuf = gl == 3 ? pbuf ^ 1 : pbuf;                     // A fragments of the next group: next chunk after gl 3
    constexpr int agl = (gl + 1) & 3;
    const float* pb = bbuf + (gl & 1) * BG_FLOATS + b_lane;
    const float* pa = patch + abuf * PATCH_FLOATS + a_lane + agl * 8;
    f32x4 b0[2], b1[2];
    b0[0] = *reinterpret_cast<const f32x4*>(pb);
    b0[1] = *reinterpret_cast<const f32x4*>(pb + 256);
    static_for<16>([&](auto fc) {
      constexpr int f = decltype(fc)::value;
      f32x4 (&bc)[2] = (f & 1) ? b1 : b0;
      f32x4 (&bn)[2] = (f & 1) ? b0 : b1;
      const f32x2 a = vv[gl & 1][f];
      // 8 MFMAs; after each one a small piece of the other work, pinned in place, so that every non-MFMA instruction
      // issues in the shadow of an executing MFMA (one wave per SIMD: nothing else would fill the gap)
      static_for<8>([&](auto kc) {
        constexpr int k = decltype(kc)::value, j = k >> 2, nb = k & 3;
        mfma_named<16 * f + 4 * nb, kFirst && j == 0>(a[j], bc[nb >> 1][(nb & 1) * 2 + j]);
        if constexpr (k == 0 && f < 15) bn[0] = *reinterpret_cast<const f32x4*>(pb + ((f + 1) * 2) * 256);
        if constexpr (k == 1 && f < 15) bn[1] = *reinterpret_cast<const f32x4*>(pb + ((f + 1) * 2 + 1) * 256);
        if constexpr (f < 4) {                                      // patch row f of the next group: 4 x b64 over two gaps
          if constexpr (k == 2) load_patch(pa, f, 0);
          if constexpr (k == 3) load_patch(pa, f, 2);
        }
        if constexpr (f == 5 && k == 2) transform_into(vv[(gl + 1) & 1]);   // patch rows landed (read at f < 4): B^T d B, all of it
        // staging: the next group's filter image first, then this group's part of a later patch chunk (see above)
        if constexpr (f == 0) {
          if (bnext) dma_piece(bimg, (gl + 1) & 1, k);
        }
        if constexpr (f == 1 && k >= 4 && gl != 2) {
          constexpr int part = gl == 3 ? 0 : gl + 1;
          if (RES && !RUNON && gl == 0 && pf_res) patch_dma_from(rsr_pf, pvl[part * 4 + (k - 4)], psoff, pbuf ^ 1, part * 4 + (k - 4));
          else patch_dma(pvl[part * 4 + (k - 4)], psoff, gl == 3 ? pbuf : pbuf ^ 1, part * 4 + (k - 4));
        }
        if constexpr (RES && RUNON && gl == 0 && f == 2 && k < 2)    // the residual lines, behind this group's patch part
          junk[k] = __builtin_amdgcn_raw_buffer_load_b32(rsr_pf, pfv[k], 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      });
    });
    // group end: the filter image (and, after group 2, the whole next patch chunk) has landed; the patch part issued in
    // this group stays in flight.  Wait and barrier are ONE asm with a memory clobber (no LDS access moves across it):
    // through __syncthreads() or a workgroup fence hipcc waits vmcnt(0) here, the DMA being an LDS write to it.
    // (a chunk's last group also lets its MFMAs land: nothing but these nops stands between a tile's last MFMA and the epilogue's first
    //  v_accvgpr_read)
    // (RUNON + RES: group 0's two residual-line loads are younger than its patch part -- six loads stay in flight; they have landed
    //  by the end of group 1, and only behind group 2's vmcnt(0) are their registers let go)
    if constexpr (gl == 3) asm volatile("s_nop 15\n\ts_nop 15\n\ts_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(gl == 2 ? 0 : (RES && RUNON && gl == 0) ? 6 : 4) : "memory");
    if constexpr (RES && RUNON && gl == 2) asm volatile("" ::"v"(junk[0]), "v"(junk[1]));
  };

  for (;;) {                                                        // the workgroup's tiles: one, or (RUNON) lt, lt + gridDim.x, ...
    using T = std::true_type;
    using F = std::false_type;
    if constexpr (!RUNON) {
#pragma unroll
      for (int j = 0; j < PDMA; ++j) pvl[j] = pv[j];
    }
    for (int chunk = 0; chunk < NCH; ++chunk) {                     // 32 channels
      const bool lastc = chunk + 1 == NCH;
      const unsigned ug = (unsigned)(ct * G + chunk * 4) * (BG_FLOATS * 4), gb = BG_FLOATS * 4;
      unsigned soff = (unsigned)((chunk + 1) * 128), soff3 = soff + 128;   // channel offsets of what groups 0, 1 / group 3 fetch
      unsigned bimg3 = ug + 4 * gb;                                 // group 3: the next chunk's first filter image
      bool bnext3 = !lastc;
      if constexpr (RUNON) {
        // the chunks of the workgroup's tiles are ONE stream (NCH >= 2): groups 0, 1 fetch parts 1, 2 of the stream's next chunk, group 3
        // part 0 of the one after it and the next group's filter image -- in a tile's last two chunks these belong to the next tile
        // (behind the last tile pvn is all kOob: the DMA writes zeros into the idle buffer, as in a one-tile launch)
        const bool nextc = chunk + 2 >= NCH;
#pragma unroll
        for (int j = 0; j < 4; ++j) pvl[j] = nextc ? pvn[j] : pv[j];
#pragma unroll
        for (int j = 4; j < PDMA; ++j) pvl[j] = lastc ? pvn[j] : pv[j];
        soff = lastc ? 0u : soff;
        soff3 = nextc ? (unsigned)((chunk + 2 - NCH) * 128) : soff3;
        bimg3 = lastc ? (unsigned)(ctn * G) * (BG_FLOATS * 4) : bimg3;
        bnext3 = !lastc || has_next;
        if constexpr (RES) {
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) pfv[s2] = kOob;
          if (lastc) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) pfv[s2] = res_line(s2, n, rb, hw, bx, ct);
          }
        }
      } else {
        if (lastc) {                                                // no next chunk: out-of-range VGPR offsets, the DMA writes zeros
#pragma unroll                                                      // into the idle buffer (the SGPR offset is not range-checked)
          for (int j = 4; j < PDMA; ++j) pvl[j] = kOob;
          if constexpr (RES) {                                      // ... except the two residual-prefetch slots (see rsr_pf)
            pf_res = true;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              // (the group adds soff to every address of this part: taken off here; an offset below soff wraps out of range and that
              //  one line is simply not prefetched)
              const unsigned ro = res_line(s2, n, rb, hw, bx, ct);
              pvl[4 + s2] = ro != kOob ? ro - soff : kOob;
            }
          }
        }
        if (chunk + 2 >= NCH) {                                     // no chunk after next: the same for the part group 3 fetches
#pragma unroll
          for (int j = 0; j < 4; ++j) pvl[j] = kOob;
        }
      }
      if (chunk == 0) group(ic<0>{}, T{}, soff, ug + 1 * gb, true); else group(ic<0>{}, F{}, soff, ug + 1 * gb, true);
      group(ic<1>{}, F{}, soff, ug + 2 * gb, true);
      group(ic<2>{}, F{}, soff, ug + 3 * gb, true);
      group(ic<3>{}, F{}, soff3, bimg3, bnext3);
      pbuf ^= 1;
    }

    // (the last, all-out-of-range patch part: LDS is reused below.  RUNON: what is in flight here is the next tile's, and stays so)
    if (!RUNON || !has_next) asm volatile("s_waitcnt vmcnt(0)");
    stamp(3);
    if constexpr (STATS || BNB != 0) __syncthreads();              // ... by EVERY wave's zero-writing DMAs before any wave's partial sums land there
    // ---- epilogue: output transform per (tile, channel), scale/shift (+res) (+relu), store ----------------------------
    // acc[f][nb][r]: tile 4 kq + r of this wave = (tile row kq>>1, tile column 4 (kq&1) + r), channel ct*64 + nb*16 + (lane&15)
    {
      // (GEO 1: tile 4 kq + r = tile row kq of the wave's four, tile column r)
      // this lane's two pixel rows (oy even, HS even: both in the same image); a row may be dead (below the map, or the row between
      // two stacked images): its base offset is out of range and every access through it is dropped by the buffer hardware
      int oy = rb + (GEO ? 8 * wave + 2 * kq : 4 * wave + 2 * (kq >> 1));
      const int ox = GEO ? 8 * bx : 16 * bx + 8 * (kq & 1);
      const bool wr = wrap_row(oy, hw);
      const int nl = n + (wr ? 1 : 0);
      const bool rok[2] = {nl < p.N && oy < p.H, nl < p.N && oy + 1 < p.H};
      const bool interior = BWP * bx + BWP <= p.W && ct * 64 + 64 <= p.Cout;
      const __amdgpu_buffer_rsrc_t rsy = buf_rsrc(p.y);
      const __amdgpu_buffer_rsrc_t rsr = buf_rsrc(p.res);
      const unsigned y_lane = (unsigned)((((nl * p.H + oy) * p.W + ox) * p.y_cs + ct * 64 + t) * 4);
      const unsigned r_lane = (unsigned)((((nl * p.H + oy) * p.W + ox) * p.res_cs + ct * 64 + t) * 4);
      const unsigned yb[2] = {rok[0] ? y_lane : kOob, rok[1] ? y_lane + (unsigned)(p.W * p.y_cs * 4) : kOob};
      const unsigned rbs[2] = {rok[0] ? r_lane : kOob, rok[1] ? r_lane + (unsigned)(p.W * p.res_cs * 4) : kOob};
      // interior tile blocks (all columns and all 64 channels exist; rows go by the two lane bases): no per-element predicate at
      // all; the scalar part of every address is an SGPR offset.  Edge blocks: out-of-range elements get an out-of-range VGPR offset.
      auto emit = [&](auto interiorc) {
        constexpr bool kInt = decltype(interiorc)::value;
        float sc[4], sh[4];
        bool cok[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          const int co = ct * 64 + nb * 16 + t;
          cok[nb] = kInt || co < p.Cout;
          sc[nb] = (p.scale && cok[nb]) ? p.scale[co] : 1.f;
          sh[nb] = (p.shift && cok[nb]) ? p.shift[co] : 0.f;
        }
        auto colok = [&](int nb, int q) {                            // q = r*4 + i*2 + j: pixel row i, column 2r + j of the lane's 2 x 8
          return kInt || (cok[nb] && ox + 2 * (q >> 2) + (q & 1) < p.W);
        };
        auto live = [&](int nb, int q) { return rok[(q >> 1) & 1] && colok(nb, q); };
        auto vo = [&](int nb, int q, const unsigned (&base)[2]) { return colok(nb, q) ? base[(q >> 1) & 1] : kOob; };
        auto soff_of = [&](int nb, int q, int cs) {                  // scalar byte offset of element q of channel block nb (within its row)
          return (unsigned)(((2 * (q >> 2) + (q & 1)) * cs + nb * 16) * 4);
        };
        float rv[2][16];                                             // residual: two channel blocks in flight
        float lx[BNB ? 2 : 1][16], ly[BNB == 2 ? 2 : 1][16];         // BNB: the BatchNorm layer's raw input / its output
        const __amdgpu_buffer_rsrc_t rbx = buf_rsrc(p.bnb_x);
        const __amdgpu_buffer_rsrc_t rby = buf_rsrc(p.bnb_y);
        auto fetch = [&](int nb, int set) {                          // BNB: one channel block's operands, a block ahead of their use
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const unsigned vy = vo(nb, q, yb);                       // bnb_x / bnb_y are laid out like y (y_cs == Cout)
            lx[set][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rbx, vy, soff_of(nb, q, p.y_cs), 0));
            if constexpr (BNB == 2)
              ly[set][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rby, vy, soff_of(nb, q, p.y_cs), 0));
            if constexpr (RES)
              rv[set][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                               rsr, vo(nb, q, rbs), soff_of(nb, q, p.res_cs), 0));
          }
        };
        // (the same residual load as in fetch, which interleaves it with its own loads: sharing the text, as a call behind fetch's loop or
        //  as a one-element helper, re-allocated the BNB + RES instantiations from their first instruction -- DESIGN 3.1b, "Deviations")
        auto res_fetch = [&](int nb, int set) {
#pragma unroll
          for (int q = 0; q < 16; ++q)
            rv[set][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsr, vo(nb, q, rbs), soff_of(nb, q, p.res_cs), 0));
        };
        if constexpr (BNB != 0) {
          fetch(0, 0);
        } else if constexpr (RES) {                                  // the residual of channel blocks 0, 1 now, of 2, 3 as their sets
          res_fetch(0, 0);                                           // free up (L2 hits: the last chunk prefetched the lines); 32
          res_fetch(1, 1);                                           // registers instead of 64
        }
        static_for<4>([&](auto nbc) {
          constexpr int nb = decltype(nbc)::value;
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (BNB != 0) {
            if (nb < 3) fetch(nb + 1, (nb + 1) & 1);
          }
          const int set = nb & 1;
          float st1 = 0.f, st2 = 0.f;                                // STATS / BNB: this lane's sums for channel nb*16 + t
          const int cch = ct * 64 + nb * 16 + t;
          const float pvt = (STATS && p.pivot && cok[nb]) ? p.pivot[cch] : 0.f;
          float mu = 0.f, is = 1.f, fa = 1.f, fb = 0.f;
          if constexpr (BNB != 0) {
            if (cok[nb]) {
              mu = p.bnb_mean[cch];
              is = p.bnb_invstd[cch];
              fa = (p.bnb_gamma ? p.bnb_gamma[cch] : 1.f) * is;
              fb = (p.bnb_beta ? p.bnb_beta[cch] : 0.f) - mu * fa;
            }
          }
          // A^T M over the frequency rows, all four tiles r at once -- as two-float halves with the subtractions as explicit packed
          // instructions: left to hipcc every vector subtraction here became scalar v_sub_f32 (192 per epilogue beside fp32 MFMAs' shared pipe)
          // (acc[f][nb][r] = accumulator register 16 f + 4 nb + r, read here)
          f32x2 sr[2][4][2];
          static_for<8>([&](auto nhc) {
            constexpr int nu = decltype(nhc)::value >> 1, hh = decltype(nhc)::value & 1;
            constexpr int r0 = 16 * nu + 4 * nb + 2 * hh;
            const f32x2 m0 = {acc_named<r0>(), acc_named<r0 + 1>()}, m1 = {acc_named<r0 + 64>(), acc_named<r0 + 65>()};
            const f32x2 m2 = {acc_named<r0 + 128>(), acc_named<r0 + 129>()}, m3 = {acc_named<r0 + 192>(), acc_named<r0 + 193>()};
            sr[0][nu][hh] = m0 + m1 + m2;
            sr[1][nu][hh] = pk_sub<false>(pk_sub<false>(m1, m2), m3);
          });
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            f32x2 yh[2][2];                                          // [j][half]
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
              yh[0][hh] = sr[i][0][hh] + sr[i][1][hh] + sr[i][2][hh];
              yh[1][hh] = pk_sub<false>(pk_sub<false>(sr[i][1][hh], sr[i][2][hh]), sr[i][3][hh]);
            }
            const f32x2 sc2 = {sc[nb], sc[nb]}, sh2 = {sh[nb], sh[nb]};
            f32x2 of[2][2];                                          // folded BatchNorm on pairs (v_pk_fma_f32)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int hh = 0; hh < 2; ++hh) of[j][hh] = __builtin_elementwise_fma(yh[j][hh], sc2, sh2);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int q = r * 4 + i * 2 + j;
                float o = of[j][r >> 1][r & 1];
                if constexpr (RES) o += rv[set][q];
                if constexpr (RELU) o = fmaxf(o, 0.f);
                if constexpr (BNB != 0) {                             // the consumer's ReLU mask, then its backward sums
                  const float tv = BNB == 2 ? ly[BNB == 2 ? set : 0][q] : fmaf(lx[set][q], fa, fb);
                  o = tv > 0.f ? o : 0.f;
                  if (live(nb, q)) {
                    st1 += o;
                    st2 = fmaf(o, (lx[set][q] - mu) * is, st2);
                  }
                }
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), rsy, vo(nb, q, yb), soff_of(nb, q, p.y_cs), 0);
                if constexpr (STATS) {
                  const float dv = live(nb, q) ? o - pvt : 0.f;
                  st1 += dv;
                  st2 = fmaf(dv, dv, st2);
                }
              }
          }
          if constexpr (RES && BNB == 0) {
            if (nb < 2) res_fetch(nb + 2, set);
          }
          if constexpr (STATS || BNB != 0) {                        // the four lane groups kq hold the same channel: fixed xor tree
            st1 += __shfl_xor(st1, 16); st2 += __shfl_xor(st2, 16);
            st1 += __shfl_xor(st1, 32); st2 += __shfl_xor(st2, 32);
            if (kq == 0) {                                          // per-wave sums -> LDS (the patch buffers are dead by now)
              lds[(wave * 64 + nb * 16 + t) * 2] = st1;
              lds[(wave * 64 + nb * 16 + t) * 2 + 1] = st2;
            }
          }
        });
      };
      if (interior) emit(std::true_type{}); else emit(std::false_type{});
      if constexpr (DIAG) {
        stamp(4);                                                   // everything issued ...
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(5);                                                   // ... and every store acknowledged
      }
      if constexpr (STATS || BNB != 0) {                            // one partial row per tile block: the four waves' sums in fixed order
        __syncthreads();
        if (tid < 64 && ct * 64 + tid < p.Cout) {
          float a1 = 0.f, a2 = 0.f;
#pragma unroll
          for (int w = 0; w < 4; ++w) { a1 += lds[(w * 64 + tid) * 2]; a2 += lds[(w * 64 + tid) * 2 + 1]; }
          float* dst = p.stats + ((size_t)(blockIdx.y * p.TBX + blockIdx.x) * p.Cout + ct * 64 + tid) * 2;
          dst[0] = a1;
          dst[1] = a2;
        }
      }
    }
    if constexpr (!RUNON) {
      break;
    } else {
      // on to the next tile: its chunk-0 patch, its first filter image and its group-0 A fragments (vv[0]) are in place or in flight
      if (!has_next) break;
      lt += (int)gridDim.x;
      n = nn; rb = rbn; hw = hwn; bx = bxn; ct = ctn;
#pragma unroll
      for (int j = 0; j < PDMA; ++j) pv[j] = pvn[j];
      make_next();
    }
  }
}


// OHWI filters [Cout][3][3][Cin] -> U image [ct][G][16 f][2 np][4 kq][16 n][2 nbl][2 cin]; U = G g G^T in double
__global__ __launch_bounds__(256) void wino_filter_transform(const float* __restrict__ w, float* __restrict__ u, int Cout,
                                                             int Cin, int nct) {
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  const long long total = (long long)nct * 64 * Cin;
  if (idx >= total) return;
  const int ci = (int)(idx % Cin), co = (int)(idx / Cin);
  double g[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) g[i][j] = co < Cout ? (double)w[(((size_t)co * 3 + i) * 3 + j) * Cin + ci] : 0.0;
  const double Gm[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
  double tmp[4][3], U[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) tmp[i][j] = Gm[i][0] * g[0][j] + Gm[i][1] * g[1][j] + Gm[i][2] * g[2][j];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) U[i][j] = tmp[i][0] * Gm[j][0] + tmp[i][1] * Gm[j][1] + tmp[i][2] * Gm[j][2];
  const int G = Cin >> 3, ct = co >> 6, nb = (co & 63) >> 4, nn = co & 15, g8 = ci >> 3, q = ci & 7;
#pragma unroll
  for (int f = 0; f < 16; ++f)
    u[((((size_t)ct * G + g8) * 16 + f) * 2 + (nb >> 1)) * 256 + ((q >> 1) * 16 + nn) * 4 + (nb & 1) * 2 + (q & 1)] =
        (float)U[f >> 2][f & 3];
}

}  // namespace

// Diagnostic / tests: workgroups of the run-on launches (0 = one per compute unit); a count at or above a launch's tile count gives the
// one-tile-per-workgroup launch
static int g_wino_workgroups = 0;
extern "C" int bevf_debug_wino_workgroups(int n) {
  BEVF_REQUIRE(n >= 0, "bevf_debug_wino_workgroups: n=%d < 0", n);
  g_wino_workgroups = n;
  return BEVF_OK;
}

// Compute units of the current device, asked once per device
static int wino_cu_count(int* out) {
  static std::mutex mu;
  static std::map<int, int> known;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lock(mu);
    const auto it = known.find(dev);
    if (it != known.end()) {
      *out = it->second;
      return BEVF_OK;
    }
    int cus = 0;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess && cus > 0) {
      known[dev] = cus;
      *out = cus;
      return BEVF_OK;
    }
  }
  (void)hipGetLastError();
  bevf_set_error("conv_wino: cannot read the device's compute-unit count: %s", hipGetErrorString(e));
  return BEVF_ERR_LAUNCH;
}

static unsigned long long* g_wino_stamps = nullptr;
// Diagnostic (tools/wino_stamps.py): buf = device buffer of 6 x 8 bytes (kWinoStamps) per workgroup of the NEXT plain launches (relu, optional residual),
// or null to stop
extern "C" int bevf_debug_wino_stamps(void* buf) {
  g_wino_stamps = static_cast<unsigned long long*>(buf);
  return BEVF_OK;
}

extern "C" int bevf_wino_stat_rows(int N, int H, int W) { return N * ((H + 15) / 16) * ((W + 15) / 16); }

extern "C" size_t bevf_wino_filter_floats(int Cout, int Cin) {
  return (size_t)((Cout + 63) / 64) * 64 * 16 * (size_t)Cin;
}

extern "C" int bevf_wino_filter_transform_f32(const float* w_ohwi, float* u, int Cout, int Cin, void* stream) {
  BEVF_REQUIRE(w_ohwi && u, "wino_filter_transform: null pointer");
  BEVF_REQUIRE(Cout > 0 && Cin > 0 && Cin % 32 == 0, "wino_filter_transform: Cin=%d must be a positive multiple of 32", Cin);
  const int nct = (Cout + 63) / 64;
  const long long total = (long long)nct * 64 * Cin;
  return bevf_launch("bevf_wino_filter_transform_f32", wino_filter_transform, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w_ohwi, u, Cout, Cin, nct);
}

extern "C" int bevf_conv3x3_wino_f32(const bevf_conv_desc* d, void* stream) {
  BEVF_REQUIRE(d && d->x && d->w && d->y, "conv_wino: null x / w / y");
  BEVF_REQUIRE(d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1, "conv_wino: 3x3, stride 1, pad 1 only (got %dx%d s%d p%d)",
               d->KH, d->KW, d->stride, d->pad);
  BEVF_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cout > 0 && d->Ho == d->H && d->Wo == d->W, "conv_wino: bad shape");
  BEVF_REQUIRE(d->Cin > 0 && d->Cin % 32 == 0, "conv_wino: Cin=%d must be a positive multiple of 32", d->Cin);
  BEVF_REQUIRE(d->x_cs >= d->Cin && d->x_cs % 4 == 0 && d->y_cs >= d->Cout, "conv_wino: channel strides");
  BEVF_REQUIRE(!d->res || d->res_cs >= d->Cout, "conv_wino: res_cs < Cout");
  BEVF_REQUIRE(!d->colmax, "conv_wino: the fused column max belongs to the 1x1 layers (bevf_conv2d_nhwc_f32)");
  BEVF_REQUIRE(bevf_aligned16(d->x) && bevf_aligned16(d->w), "conv_wino: x / w must be 16-byte aligned");
  BEVF_REQUIRE((long long)d->N * d->H * d->W * d->x_cs * 4 < (1ll << 31) && (long long)d->N * d->H * d->W * d->y_cs * 4 < (1ll << 31) &&
                   (!d->res || (long long)d->N * d->H * d->W * d->res_cs * 4 < (1ll << 31)),
               "conv_wino: activations must stay below 2 GiB (32-bit buffer offsets)");
  BEVF_REQUIRE((long long)((d->Cout + 63) / 64) * 64 * 16 * d->Cin * 4 < (1ll << 31), "conv_wino: transformed filters must stay below 2 GiB");
  WinoArgs a;
  a.x = d->x; a.u = d->w; a.scale = d->scale; a.shift = d->shift; a.res = d->res; a.y = d->y;
  a.stats = d->stats; a.pivot = d->stats_pivot;
  a.bnb_x = d->bnb_x; a.bnb_y = d->bnb_y; a.bnb_mean = d->bnb_mean; a.bnb_invstd = d->bnb_invstd;
  a.bnb_gamma = d->bnb_gamma; a.bnb_beta = d->bnb_beta;
  if (d->bnb_x) {
    BEVF_REQUIRE(d->stats && d->bnb_mean && d->bnb_invstd && !d->relu && !d->stats_pivot && d->y_cs == d->Cout,
                 "conv_wino: the BatchNorm-backward epilogue needs stats (partials out), mean, invstd, relu = 0 and y_cs == Cout");
  } else {
    BEVF_REQUIRE(!d->stats || (!d->res && !d->relu), "conv_wino: stats need relu = 0 and no residual (they describe the raw conv output)");
  }
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.x_cs = d->x_cs; a.Cout = d->Cout; a.y_cs = d->y_cs; a.res_cs = d->res_cs;
  a.TBY = (d->H + 15) / 16; a.TBX = (d->W + 15) / 16; a.nct = (d->Cout + 63) / 64;
  a.HS = 0; a.SB = d->N * a.TBY; a.stamps = nullptr;
  // Block geometry (16x16 or 32x8 pixels) and row stacking (WinoArgs::HS): whichever covers the batch with the fewest blocks; plain
  // epilogues only (the statistics rows are per 16x16 block of one image).  tile: 0 = auto, 1 / 2 = 16x16 / 32x8 per image,
  // 3 / 4 = the same two over stacked rows (tests: all four are bit-identical)
  bool geo1 = false;
  if (!d->stats && !d->bnb_x && d->tile != 1) {
    const int hs = d->H + 1 + ((d->H + 1) & 1);                     // even, >= H + 1
    long long best = (long long)a.SB * a.TBX;
    for (int cand = 1; cand < 4; ++cand) {                          // bit 0: 32x8 blocks, bit 1: stacked rows
      const int bh = (cand & 1) ? 32 : 16, bw = (cand & 1) ? 8 : 16, tbx = (d->W + bw - 1) / bw;
      if ((cand & 2) && (hs <= bh || (long long)d->N * hs >= (1ll << 30))) continue;
      const long long sb = (cand & 2) ? ((long long)d->N * hs - (hs - d->H) + bh - 1) / bh : (long long)d->N * ((d->H + bh - 1) / bh);
      const bool forced = d->tile == cand + 1;
      if (d->tile != 0 && !forced) continue;
      if (forced || sb * tbx < best) {
        best = sb * tbx;
        geo1 = cand & 1;
        a.TBY = (d->H + bh - 1) / bh; a.TBX = tbx; a.SB = (int)sb; a.HS = (cand & 2) ? hs : 0;
      }
    }
  }
  const long long ntiles = (long long)a.SB * a.TBX * a.nct;
  BEVF_REQUIRE(ntiles < (1ll << 31) && a.SB < 65536 && a.nct < 65536, "conv_wino: too many tiles");
  {                                                                 // row -> image by multiply-high: exact while (rows + divisor) * divisor < 2^32
    const unsigned long long dv = a.HS ? (unsigned long long)a.HS : (unsigned long long)a.TBY;
    const unsigned long long top = a.HS ? (unsigned long long)a.SB * (geo1 ? 32 : 16) + dv : (unsigned long long)a.SB;
    BEVF_REQUIRE((top + dv) * dv < (1ull << 32), "conv_wino: map too tall for the row arithmetic");
    a.div_mul = (unsigned)(((1ull << 32) + dv - 1) / dv);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  dim3 grid((unsigned)a.TBX, (unsigned)a.SB, (unsigned)a.nct);
  const dim3 block(256);
  const bool diag = g_wino_stamps && d->relu;                      // diagnostic launch: same kernel, six time stamps per workgroup
  // Run-on launch (plain epilogues, at least two patch chunks): one workgroup per compute unit, each walking tiles b, b + G, ... -- when
  // that is fewer workgroups than tiles and the tile decode's multiply-high is exact ((n + d) * d < 2^32 for both divisors)
  a.ntiles = (int)ntiles; a.nsp = a.SB * a.TBX; a.nsp_mul = a.tbx_mul = 0;
  bool runon = false;
  if (!d->stats && !d->bnb_x && !diag && d->Cin >= 64) {
    int wgs = g_wino_workgroups;
    bool pays = true;
    if (wgs == 0) {
      const int rc = wino_cu_count(&wgs);
      if (rc != BEVF_OK) return rc;
      // The fixed tile -> workgroup assignment gives up the dispatcher's balancing: with few, uneven rounds per compute unit the idle
      // tail costs more than the run-on saves (measured: 2.8 rounds + 1.0 %, 4.8 rounds + 0.5 %; 8.7 rounds - 3 %, 4 whole rounds
      // - 9 %; profiles/r10_wino_cells.txt).  A forced count is taken as given.
      pays = ntiles % wgs == 0 || ntiles >= 8ll * wgs;
    }
    const unsigned long long nsp = (unsigned long long)a.nsp, tbx = (unsigned long long)a.TBX;
    if (pays && wgs < ntiles && ((unsigned long long)ntiles + nsp) * nsp < (1ull << 32) && (nsp + tbx) * tbx < (1ull << 32)) {
      runon = true;
      if (nsp > 1) a.nsp_mul = (unsigned)(((1ull << 32) + nsp - 1) / nsp);
      if (tbx > 1) a.tbx_mul = (unsigned)(((1ull << 32) + tbx - 1) / tbx);
      grid = dim3((unsigned)wgs);
    }
  }
  auto go = [&](auto kern) { return bevf_launch("bevf_conv3x3_wino_f32", kern, grid, block, LDS_BYTES, st, a); };
  // the launchable instantiations of wino_f32<RES, RELU, STATS, BNB, GEO, DIAG, RUNON>: BNB 1 / 2 x RES, STATS, DIAG x RES x GEO,
  // plain RES x RELU x GEO x RUNON
  if (d->bnb_x)
    return bevf_dispatch_bool(d->res != nullptr, [&](auto R) {
      constexpr bool res = decltype(R)::value;
      return d->bnb_y ? go(&wino_f32<res, false, false, 2>) : go(&wino_f32<res, false, false, 1>);
    });
  if (d->stats) return go(&wino_f32<false, false, true>);
  if (diag) a.stamps = g_wino_stamps;
  return bevf_dispatch_bool(d->res != nullptr, [&](auto R) {
    return bevf_dispatch_bool(geo1, [&](auto G) {
      constexpr bool res = decltype(R)::value;
      constexpr int geo = decltype(G)::value;
      if (diag) return go(&wino_f32<res, true, false, 0, geo, true>);
      return bevf_dispatch_bool(runon, [&](auto O) {
        constexpr bool ro = decltype(O)::value;
        return d->relu ? go(&wino_f32<res, true, false, 0, geo, false, ro>) : go(&wino_f32<res, false, false, 0, geo, false, ro>);
      });
    });
  });
}
