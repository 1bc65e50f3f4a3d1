// Rotated-rectangle geometry shared by the box kernels (box_nms.hip: pairwise IoU and NMS; iou_loss.hip: IoU targets of the
// IoU-aware head).  Internal header; the derivation of the clipping is at the top of box_nms.hip.
#pragma once
#include "common.h"

namespace {

struct RBox {
  float x, y, c, s, hl, hw, area;   // centre, heading (cos, sin), half extents along / across the heading, l * w
  float z, h;
  int ok;                           // w > 0 and l > 0 (false for NaN)
};

__device__ __forceinline__ RBox load_box(const float* p) {
  RBox r;
  r.x = p[0]; r.y = p[1]; r.z = p[2];
  const float w = p[3], l = p[4];
  r.h = p[5];
  sincosf(p[6], &r.s, &r.c);
  r.hl = 0.5f * l; r.hw = 0.5f * w;
  r.area = l * w;
  r.ok = (w > 0.f) && (l > 0.f);
  return r;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// -dx * integral of clamp(y, -hy, hy) over the part of the edge p -> q inside |x| <= hx
__device__ __forceinline__ float edge_term(float px, float py, float qx, float qy, float hx, float hy) {
  const float dx = qx - px, dy = qy - py;
  if (dx == 0.f) return 0.f;
  const float ta = (-hx - px) / dx, tb = (hx - px) / dx;
  const float t0 = clampf(fminf(ta, tb), 0.f, 1.f), t1 = clampf(fmaxf(ta, tb), 0.f, 1.f);
  float integ;
  if (dy == 0.f) {
    integ = clampf(py, -hy, hy) * (t1 - t0);
  } else {
    const float ua = (-hy - py) / dy, ub = (hy - py) / dy;
    const float u = clampf(fminf(ua, ub), t0, t1), v = clampf(fmaxf(ua, ub), t0, t1);
    const float c1 = dy > 0.f ? -hy : hy;                       // y is clamped there before the edge enters |y| <= hy
    integ = c1 * (u - t0) + (v - u) * (py + dy * (0.5f * (u + v))) - c1 * (t1 - v);
  }
  return -dx * integ;
}

// area of the intersection of the two rectangles, in [0, min(area_a, area_b)]; 0 for NaN
__device__ __forceinline__ float inter_area(const RBox& a, const RBox& b) {
  const float tx = b.x - a.x, ty = b.y - a.y;
  const float cx = a.c * tx + a.s * ty, cy = a.c * ty - a.s * tx;          // b's centre in a's frame
  const float dc = b.c * a.c + b.s * a.s, ds = b.s * a.c - b.c * a.s;      // b's heading in a's frame
  const float lx = b.hl * dc, ly = b.hl * ds, wx = -b.hw * ds, wy = b.hw * dc;
  const float x0 = cx + lx + wx, y0 = cy + ly + wy;                        // counter-clockwise corners
  const float x1 = cx - lx + wx, y1 = cy - ly + wy;
  const float x2 = cx - lx - wx, y2 = cy - ly - wy;
  const float x3 = cx + lx - wx, y3 = cy + ly - wy;
  float s = edge_term(x0, y0, x1, y1, a.hl, a.hw);
  s += edge_term(x1, y1, x2, y2, a.hl, a.hw);
  s += edge_term(x2, y2, x3, y3, a.hl, a.hw);
  s += edge_term(x3, y3, x0, y0, a.hl, a.hw);
  const float cap = fminf(a.area, b.area);
  return (s > 0.f) ? fminf(s, cap) : 0.f;                                  // NaN compares false -> 0
}

__device__ __forceinline__ float unit(float v) { return (v > 0.f) ? fminf(v, 1.f) : 0.f; }   // clamp to [0,1], NaN -> 0

__device__ __forceinline__ float iou_bev(const RBox& a, const RBox& b) {
  if (!(a.ok && b.ok)) return 0.f;
  const float inter = inter_area(a, b);
  return unit(inter / (a.area + b.area - inter));
}

__device__ __forceinline__ float iou_3d(const RBox& a, const RBox& b) {
  if (!(a.ok && b.ok && a.h > 0.f && b.h > 0.f)) return 0.f;
  const float inter = inter_area(a, b);
  const float dz = b.z - a.z;                                              // b's z in a's frame
  const float zo = fminf(0.5f * a.h, dz + 0.5f * b.h) - fmaxf(-0.5f * a.h, dz - 0.5f * b.h);
  const float iv = (zo > 0.f) ? inter * fminf(zo, fminf(a.h, b.h)) : 0.f;
  return unit(iv / (a.area * a.h + b.area * b.h - iv));
}

}  // namespace
