// Map polygons and polylines rasterised into segmentation targets: the (B, K, Ho, Wo) uint8 masks of the BEV
// map-segmentation head from vector geometry, after the step's world transform.
//   map_raster_shapes   pre-pass, one wave per shape: every vertex through the frame's transform in fp64 (never rounded back to fp32)
//                       and, into the workspace, one 32-byte EDGE per vertex -- the edge from that vertex to the next one of its ring,
//                       a polygon's already turned so that a is the lower end (a horizontal one, and the slot behind a polyline's
//                       last vertex, hold values no cell can satisfy) -- and one 64-byte record per shape: the fp64 box of the
//                       transformed vertices -- widened by a polyline's half width and a rounding allowance, never shrunk --, class,
//                       kind, edge range and half width.  Every offset and index is checked HERE, on the device, against the array
//                       sizes; a shape that fails a check, has a non-finite transformed vertex or too few vertices gets an empty box
//                       and is never looked at again.
//   map_raster_fill     main pass, one 256-thread workgroup per tile of 32 x 32 cells of one frame; a lane owns four adjacent cells
//                       of one row.  The frame's shape records are tested against the tile's span of cell centres 256 at a time (one
//                       per thread, survivors compacted in order through LDS with a running sum of their edge counts); the
//                       survivors' edges, one flat sequence, are read RASTER_CHUNK at a time (one per thread) and those the tile can feel
//                       -- the same kind of box test, per edge -- are staged in LDS in order, each with a tag (class, kind, last edge of
//                       its shape); every lane tests its cells against the staged edges, UNROLL LDS reads in flight, carries the
//                       crossing parity in registers from edge to edge and chunk to chunk, and at a shape's last edge ORs the result
//                       into one 64-bit class word per cell.  The K planes leave as 4-byte stores (byte stores when Wo % 4 != 0).
// All geometry in fp64 with contraction off: a numpy fp64 restatement gives the same bytes.  No atomics, no MFMA, 19 KB of LDS.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RASTER_MAX_CLASSES = 64;   // one bit per class in a cell's word (SEG_MAX_CLASSES of bev_seg.hip)
constexpr int RASTER_CHUNK = 256;        // edges staged per round: one per thread
constexpr int TILE_W = 32, TILE_H = 32;  // cells; 8 lanes x 4 cells wide, 32 rows
constexpr int CELLS = 4;                 // adjacent cells of one row per lane
constexpr int UNROLL = 4;                // staged edges a lane reads from LDS at a time
static_assert(TILE_W / CELLS * TILE_H == 256 && RASTER_CHUNK == 256, "one lane per four cells, one staged edge per thread");
constexpr int TAG_LINE = 1 << 8, TAG_LAST = 1 << 9;   // an edge's tag: class | TAG_LINE (polyline) | TAG_LAST (closes its shape)

typedef double f64x2 __attribute__((ext_vector_type(2)));

struct ShapeRec {   // 64 bytes
  double x0, y0, x1, y1;   // widened box of the transformed vertices; an empty shape: (inf, inf, -inf, -inf)
  double hw;               // half width of a polyline after the frame's scale, 0 for a polygon
  int cls, kind, e0, e1;   // class, 0 = polygon / 1 = polyline, the shape's edges [e0, e1) (= its vertex range, checked by the pre-pass)
  double grow;             // by how much the box, and the box of each of its edges, is widened
};
static_assert(sizeof(ShapeRec) == 64, "ShapeRec is one 64-byte record");

struct RasterGrid {
  double x0, y0, vx, vy;
};

struct RasterSizes {
  int V, R, S, B, K;
};

__device__ __forceinline__ double wave_min(double v) {
  for (int m = 32; m > 0; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int m = 32; m > 0; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}

// ---- pre-pass ------------------------------------------------------------------------------------------------------------------

struct Affine2 {
  double m00, m01, m03, m10, m11, m13;
};

__device__ __forceinline__ f64x2 transformed(const Affine2& t, const float* __restrict__ vertices, int v) {
  const double x = (double)vertices[2 * (size_t)v], y = (double)vertices[2 * (size_t)v + 1];
  f64x2 p;
  p.x = (t.m00 * x + t.m01 * y) + t.m03;
  p.y = (t.m10 * x + t.m11 * y) + t.m13;
  return p;
}

// mat: fp32 [B][12] (rows 0-2 of the frame's 4x4) or null = identity; scale: fp32 [B] or null = 1.  edges [V][4] = (a.x, a.y, b.x, b.y).
__global__ __launch_bounds__(256) void map_raster_shapes(const float* __restrict__ vertices, const int* __restrict__ ring_offsets,
                                                         const int* __restrict__ shape_offsets, const int* __restrict__ shape_class,
                                                         const int* __restrict__ shape_kind, const float* __restrict__ shape_width,
                                                         const int* __restrict__ frame_offsets, const float* __restrict__ mat,
                                                         const float* __restrict__ scale, RasterSizes n, ShapeRec* __restrict__ recs,
                                                         f64x2* __restrict__ edges) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int s = (int)blockIdx.x * 4 + wave;
  if (s >= n.S) return;
  // the frame that holds shape s: the lowest b with frame_offsets[b] <= s < frame_offsets[b + 1]
  int fb = n.B;
  for (int b = lane; b < n.B; b += 64)
    if (frame_offsets[b] <= s && s < frame_offsets[b + 1]) fb = min(fb, b);
  for (int m = 32; m > 0; m >>= 1) fb = min(fb, __shfl_xor(fb, m, 64));
  const int cls = shape_class[s], kind = shape_kind[s];
  const int r0 = shape_offsets[s], r1 = shape_offsets[s + 1];
  bool ok = fb < n.B && cls >= 0 && cls < n.K && (kind == 0 || kind == 1) && r0 >= 0 && r0 < r1 && r1 <= n.R &&
            (kind == 0 || r1 - r0 == 1);
  Affine2 t{1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  double sc = 1.0;
  if (ok && mat) {
    const float* m = mat + (size_t)fb * 12;
    t = Affine2{(double)m[0], (double)m[1], (double)m[3], (double)m[4], (double)m[5], (double)m[7]};
  }
  if (ok && scale) sc = (double)scale[fb];
  const double inf = __builtin_huge_val();
  double xlo = inf, ylo = inf, xhi = -inf, yhi = -inf;
  bool finite = true;
  const int need = kind == 1 ? 2 : 3;
  int e0 = 0, e1 = 0;
  for (int r = r0; ok && r < r1; ++r) {
    const int v0 = ring_offsets[r], v1 = ring_offsets[r + 1];
    if (!(v0 >= 0 && v0 <= v1 && v1 <= n.V && v1 - v0 >= need)) {
      ok = false;
      break;
    }
    if (r == r0) e0 = v0;
    e1 = v1;   // (ring r + 1 starts where ring r ends: the shape's vertices, and so its edges, are one range)
    for (int v = v0 + lane; v < v1; v += 64) {
      f64x2 a = transformed(t, vertices, v);
      finite = finite && isfinite(a.x) && isfinite(a.y);
      xlo = fmin(xlo, a.x), xhi = fmax(xhi, a.x);
      ylo = fmin(ylo, a.y), yhi = fmax(yhi, a.y);
      f64x2 b;
      if (kind == 1 && v + 1 == v1) {
        a.x = a.y = b.x = b.y = __builtin_nan("");   // behind a polyline's last vertex: every comparison of the rule is false
      } else {
        b = transformed(t, vertices, v + 1 == v1 ? v0 : v + 1);   // the identical expression its own slot evaluates
        if (kind == 0) {
          if (a.y == b.y) {
            a.y = b.y = inf;   // a horizontal edge is skipped: a.y <= py is never true
          } else if (a.y > b.y) {
            const f64x2 c = a;
            a = b, b = c;
          }
        }
      }
      edges[2 * (size_t)v] = a;
      edges[2 * (size_t)v + 1] = b;
    }
  }
  ok = ok && __ballot(!finite) == 0ull;
  xlo = wave_min(xlo), ylo = wave_min(ylo), xhi = wave_max(xhi), yhi = wave_max(yhi);
  if (lane != 0) return;
  ShapeRec rec;
  rec.x0 = rec.y0 = inf;
  rec.x1 = rec.y1 = -inf;
  rec.hw = 0.0;
  rec.cls = rec.kind = rec.e0 = rec.e1 = 0;
  rec.grow = 0.0;
  if (ok) {
    const double hw = kind == 1 ? 0.5 * (double)shape_width[s] * sc : 0.0;
    // The box only has to be a superset of the cells the rules below can mark.  A polyline reaches fabs(hw) past its vertices; the
    // allowance on top -- 2^-20 of that reach and 2^-40 of the largest coordinate -- is orders of magnitude above the rounding of the
    // rules' own differences and products (2^-53 relative), so a cell outside the box is at a distance at which the fp64 test gives
    // what the exact one gives: no hit, and for a polygon an even number of crossings (none to the right, every edge of the row's span
    // to the left).  A NaN half width gives a NaN box, which no tile overlaps: the rules' comparisons are then false everywhere too.
    const double big = fmax(fmax(fabs(xlo), fabs(xhi)), fmax(fabs(ylo), fabs(yhi)));
    const double grow = fabs(hw) * (1.0 + 0x1p-20) + big * 0x1p-40;
    rec.x0 = xlo - grow, rec.y0 = ylo - grow, rec.x1 = xhi + grow, rec.y1 = yhi + grow;
    rec.hw = hw, rec.grow = grow;
    rec.cls = cls, rec.kind = kind, rec.e0 = e0, rec.e1 = e1;
  }
  recs[s] = rec;
}

// ---- main pass -----------------------------------------------------------------------------------------------------------------

// The centre of cell index o along one axis: the expression of axis_sample in bev_seg.hip.
__device__ __forceinline__ double cell_centre(double origin, double vox, int o) { return origin + ((double)o + 0.5) * vox; }

// VEC: Wo % 4 == 0 and a 4-byte aligned base, so a lane's four cells are inside or outside the row together and leave as one store.
template <bool VEC>
__global__ __launch_bounds__(256) void map_raster_fill(const ShapeRec* __restrict__ recs, const f64x2* __restrict__ edges,
                                                       const int* __restrict__ frame_offsets, uint8_t* __restrict__ out, RasterGrid g,
                                                       int K, int Ho, int Wo, int S, int tiles_x, int tiles_y) {
  // the staged chunk (UNROLL - 1 slots of slack: the walk reads whole groups and drops what lies past the end)
  __shared__ f64x2 lds_y[RASTER_CHUNK + UNROLL - 1], lds_x[RASTER_CHUNK + UNROLL - 1];   // (a.y, b.y), (a.x, b.x)
  __shared__ double lds_hw2[RASTER_CHUNK + UNROLL - 1];                                   // the edge's shape's squared half width
  __shared__ int lds_tag[RASTER_CHUNK + UNROLL - 1];
  __shared__ double surv_hw2[256], surv_grow[256];   // the batch's surviving shapes, in shape order: squared half width, box allowance,
  __shared__ int surv_tag[256], surv_e0[256];        // class | TAG_LINE, first edge,
  __shared__ int surv_first[257];                    // and the position of that edge in the batch's flat edge sequence ([n]: its length)
  __shared__ int wave_shapes[4], wave_edges[4], wave_kept[4];
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int bid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int per_frame = tiles_x * tiles_y;
  const int b = bid / per_frame, t = bid - b * per_frame;
  const int ti = t / tiles_x, tj = t - ti * tiles_x;
  const int i = ti * TILE_H + (tid >> 3), j0 = tj * TILE_W + (tid & 7) * CELLS;
  const double py = cell_centre(g.y0, g.vy, i);
  double px[CELLS];
#pragma unroll
  for (int c = 0; c < CELLS; ++c) px[c] = cell_centre(g.x0, g.vx, j0 + c);
  // the tile's span of centres (rows and columns inside the grid only)
  const double xa = cell_centre(g.x0, g.vx, tj * TILE_W), xb = cell_centre(g.x0, g.vx, min(tj * TILE_W + TILE_W, Wo) - 1);
  const double ya = cell_centre(g.y0, g.vy, ti * TILE_H), yb = cell_centre(g.y0, g.vy, min(ti * TILE_H + TILE_H, Ho) - 1);
  const double tx0 = fmin(xa, xb), tx1 = fmax(xa, xb), ty0 = fmin(ya, yb), ty1 = fmax(ya, yb);
  unsigned long long word[CELLS];
#pragma unroll
  for (int c = 0; c < CELLS; ++c) word[c] = 0ull;
  unsigned hit = 0u;   // bit c: cell c's crossing parity (polygon) or hit (polyline) in the shape being walked

  const int f0 = min(max(frame_offsets[b], 0), S), f1 = min(max(frame_offsets[b + 1], 0), S);
  for (int base = f0; base < f1; base += 256) {
    // one record per thread against the tile's span; survivors keep their order
    const int sl = base + tid;
    bool keep = false;
    int ne = 0;
    const ShapeRec* r = recs + sl;
    if (sl < f1) {
      keep = r->x0 <= tx1 && tx0 <= r->x1 && r->y0 <= ty1 && ty0 <= r->y1;   // (false for an empty or NaN box)
      if (keep) ne = r->e1 - r->e0;
    }
    const unsigned long long mask = __ballot(keep);
    int upto = ne;   // edges of this wave's survivors up to and including this lane's
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(upto, d, 64);
      if (lane >= d) upto += o;
    }
    if (lane == 63) wave_shapes[wave] = __builtin_popcountll(mask), wave_edges[wave] = upto;
    __syncthreads();
    int shapes_before = 0, edges_before = 0, n_shapes = 0, n_edges = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int ws = wave_shapes[w], we = wave_edges[w];
      shapes_before += w < wave ? ws : 0, edges_before += w < wave ? we : 0;
      n_shapes += ws, n_edges += we;
    }
    if (keep) {
      const int pos = shapes_before + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
      surv_first[pos] = edges_before + upto - ne;
      surv_e0[pos] = r->e0;
      surv_tag[pos] = r->cls | (r->kind == 1 ? TAG_LINE : 0);
      surv_hw2[pos] = r->hw * r->hw;
      surv_grow[pos] = r->grow;
    }
    if (tid == 0) surv_first[n_shapes] = n_edges;
    n_shapes = __builtin_amdgcn_readfirstlane(n_shapes);
    n_edges = __builtin_amdgcn_readfirstlane(n_edges);
    for (int c0 = 0; c0 < n_edges; c0 += RASTER_CHUNK) {
      const int nc = min(RASTER_CHUNK, n_edges - c0);
      __syncthreads();   // (the survivor lists are written; the previous chunk has been read)
      // One edge per thread, kept when the tile can feel it: its box, widened by its shape's allowance, must meet the tile's rows; a
      // polyline's must meet the tile's columns too; a polygon's must not lie wholly left of them -- a cell right of both ends has
      // (b.x - a.x)(py - a.y) <= (px - a.x)(b.y - a.y) factor by factor, rounding is monotone, so d > 0 cannot hold.  (An edge right
      // of the tile IS crossed by every row of its span.)  A shape's last edge is always kept: it closes the shape.
      f64x2 a{0.0, 0.0}, bb{0.0, 0.0};
      int tag = 0;
      double hw2 = 0.0;
      bool kept = false;
      if (tid < nc) {
        const int f = c0 + tid;
        int lo = 0, hi = n_shapes;   // the survivor that owns flat edge f: the last one with surv_first <= f (every shape has edges)
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (surv_first[mid] <= f) lo = mid; else hi = mid;
        }
        const size_t e = (size_t)(surv_e0[lo] + (f - surv_first[lo]));
        a = edges[2 * e], bb = edges[2 * e + 1];
        hw2 = surv_hw2[lo];
        tag = surv_tag[lo] | (f + 1 == surv_first[lo + 1] ? TAG_LAST : 0);
        const double grow = surv_grow[lo];
        const bool rows = fmin(a.y, bb.y) - grow <= ty1 && ty0 <= fmax(a.y, bb.y) + grow;
        const bool right = tx0 <= fmax(a.x, bb.x) + grow, left = fmin(a.x, bb.x) - grow <= tx1;
        kept = (tag & TAG_LAST) || (rows && right && (left || !(tag & TAG_LINE)));
      }
      const unsigned long long kmask = __ballot(kept);
      if (lane == 0) wave_kept[wave] = __builtin_popcountll(kmask);
      __syncthreads();
      int kept_before = 0, n_kept = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int wk = wave_kept[w];
        kept_before += w < wave ? wk : 0, n_kept += wk;
      }
      if (kept) {
        const int slot = kept_before + __builtin_popcountll(kmask & ((1ull << lane) - 1ull));
        lds_y[slot] = f64x2{a.y, bb.y}, lds_x[slot] = f64x2{a.x, bb.x};
        lds_hw2[slot] = hw2, lds_tag[slot] = tag;
      }
      __syncthreads();
      n_kept = __builtin_amdgcn_readfirstlane(n_kept);
      for (int e = 0; e < n_kept; e += UNROLL) {
        // a group's LDS reads go out together; the row test of every polygon edge follows before any branch
        f64x2 ys[UNROLL], xs[UNROLL];
        double h2[UNROLL];
        int tg[UNROLL];
        bool span[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) ys[u] = lds_y[e + u], xs[u] = lds_x[e + u], h2[u] = lds_hw2[e + u], tg[u] = lds_tag[e + u];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) span[u] = ys[u].x <= py && py < ys[u].y;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          if (e + u >= n_kept) break;
          const int tu = __builtin_amdgcn_readfirstlane(tg[u]);
          const double ax = xs[u].x, bx = xs[u].y, ay = ys[u].x, by = ys[u].y;
          if (!(tu & TAG_LINE)) {
            if (span[u]) {
              const double lhs = (bx - ax) * (py - ay), dy = by - ay;
#pragma unroll
              for (int c = 0; c < CELLS; ++c) {
                const double d = lhs - (px[c] - ax) * dy;
                hit ^= d > 0.0 ? 1u << c : 0u;
              }
            }
          } else {
            const double ex = bx - ax, ey = by - ay, uy = py - ay, wy = py - by;
            const double l2 = ex * ex + ey * ey, lim = h2[u] * l2;
#pragma unroll
            for (int c = 0; c < CELLS; ++c) {
              const double ux = px[c] - ax;
              const double tt = ux * ex + uy * ey;
              bool h;
              if (tt <= 0.0) {
                h = ux * ux + uy * uy <= h2[u];
              } else if (tt >= l2) {
                const double wx = px[c] - bx;
                h = wx * wx + wy * wy <= h2[u];
              } else {
                const double cr = ex * uy - ey * ux;
                h = cr * cr <= lim;
              }
              hit |= h ? 1u << c : 0u;
            }
          }
          if (tu & TAG_LAST) {
            const int cls = tu & 0xff;
#pragma unroll
            for (int c = 0; c < CELLS; ++c) word[c] |= (unsigned long long)((hit >> c) & 1u) << cls;
            hit = 0u;
          }
        }
      }
    }
    __syncthreads();   // (the survivor lists and the wave sums are rewritten by the next batch)
  }

  if (i >= Ho || j0 >= Wo) return;
  const size_t plane = (size_t)Ho * (size_t)Wo;
  uint8_t* dst = out + (size_t)b * (size_t)K * plane + (size_t)i * (size_t)Wo + (size_t)j0;
  for (int k = 0; k < K; ++k, dst += plane) {
    if (VEC) {
      unsigned v = 0u;
#pragma unroll
      for (int c = 0; c < CELLS; ++c) v |= (unsigned)((word[c] >> k) & 1ull) << (8 * c);
      *reinterpret_cast<unsigned*>(dst) = v;
    } else {
#pragma unroll
      for (int c = 0; c < CELLS; ++c)
        if (j0 + c < Wo) dst[c] = (uint8_t)((word[c] >> k) & 1ull);
    }
  }
}

size_t recs_bytes(int S) { return (size_t)(S > 0 ? S : 0) * sizeof(ShapeRec); }

}  // namespace

extern "C" size_t bevf_map_raster_work_bytes(int S, int V) { return recs_bytes(S) + (size_t)(V > 0 ? V : 0) * 2 * sizeof(f64x2); }

extern "C" int bevf_map_raster_u8(const float* vertices, int V, const int32_t* ring_offsets, int R, const int32_t* shape_offsets,
                                  const int32_t* shape_class, const int32_t* shape_kind, const float* shape_width, int S,
                                  const int32_t* frame_offsets, int B, const float* mat, const float* scale, int K, int Ho, int Wo,
                                  double x0, double y0, double vx, double vy, void* work, uint8_t* out, void* stream) {
  BEVF_REQUIRE(frame_offsets && out, "map_raster: null pointer");
  BEVF_REQUIRE(K >= 1 && K <= RASTER_MAX_CLASSES, "map_raster: K = %d classes, need 1 .. %d", K, RASTER_MAX_CLASSES);
  BEVF_REQUIRE(B > 0 && Ho > 0 && Wo > 0 && V >= 0 && R >= 0 && S >= 0, "map_raster: bad shape (B=%d Ho=%d Wo=%d V=%d R=%d S=%d)", B, Ho,
               Wo, V, R, S);
  BEVF_REQUIRE(S == 0 || (vertices && ring_offsets && shape_offsets && shape_class && shape_kind && shape_width && work),
               "map_raster: null pointer (S = %d shapes)", S);
  BEVF_REQUIRE(((uintptr_t)work & 15u) == 0, "map_raster: the workspace must be 16-byte aligned");
  const int tiles_x = (Wo + TILE_W - 1) / TILE_W, tiles_y = (Ho + TILE_H - 1) / TILE_H;
  BEVF_REQUIRE((long long)B * tiles_x * tiles_y < (1ll << 31), "map_raster: more than 2^31 tiles");
  hipStream_t st = static_cast<hipStream_t>(stream);
  ShapeRec* recs = static_cast<ShapeRec*>(work);
  f64x2* edges = reinterpret_cast<f64x2*>(static_cast<char*>(work) + recs_bytes(S));
  if (S > 0) {
    const RasterSizes n{V, R, S, B, K};
    const int rc = bevf_launch("bevf_map_raster_u8", map_raster_shapes, dim3((S + 3) / 4), dim3(256), 0, st, vertices,
                               (const int*)ring_offsets, (const int*)shape_offsets, (const int*)shape_class, (const int*)shape_kind,
                               shape_width, (const int*)frame_offsets, mat, scale, n, recs, edges);
    if (rc != BEVF_OK) return rc;
  }
  const RasterGrid g{x0, y0, vx, vy};
  const bool vec = Wo % 4 == 0 && ((uintptr_t)out & 3u) == 0;
  const dim3 grid((unsigned)(B * tiles_x * tiles_y)), block(256);
  return bevf_dispatch_bool(vec, [&](auto v) {
    return bevf_launch("bevf_map_raster_u8", map_raster_fill<decltype(v)::value>, grid, block, 0, st, (const ShapeRec*)recs,
                       (const f64x2*)edges, (const int*)frame_offsets, out, g, K, Ho, Wo, S, tiles_x, tiles_y);
  });
}
