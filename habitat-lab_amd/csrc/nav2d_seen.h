// Which cells of the Nav2D grid the camera sees from a pose: the rule of the top-down map's fog of war (csrc/nav2d_map.hip) and of
// Nav2DExplore-v0's coverage layer (csrc/nav2d.hip), written once.  Specification: tests/nav2d_map_reference.py (`occupied`,
// `reveal`).  Every float operation is one fp32 rounding in the written order: contraction is off for this code, as it is in both
// files that include it; nothing divides and nothing takes a root.  A record is read through the word offsets of
// include/habitat_amd.h alone: every Nav2D record begins with a Nav2D-v0 record.
#pragma once
#include "hab_common.h"
#include "../../include/habitat_amd.h"

#pragma clang fp contract(off)

namespace nav2d_seen {

constexpr int MAX_K = HAB_NAV2D_MAX_OBSTACLES;
constexpr float HALF = 0.5f;
constexpr float NEAR_R2 = 0.25f * 0.25f;  // a squared radius: one fp32 product of the rounded radius with itself

__device__ inline float word_f(const int32_t* w, int i) { return __int_as_float(w[i]); }

// What the rule needs of an env: the pose, the raw rectangles for the occupancy test and in the centre / half-extent form of the
// separating-axis test.
struct Sight {
    float px, py, c, s;
    float x0[MAX_K], y0[MAX_K], x1[MAX_K], y1[MAX_K];
    float cx[MAX_K], ex[MAX_K], cy[MAX_K], ey[MAX_K];
};

// Rectangle k from its raw corners.
__device__ inline void set_rect(Sight& e, int k, float lx, float ly, float hx, float hy) {
    e.x0[k] = lx; e.y0[k] = ly; e.x1[k] = hx; e.y1[k] = hy;
    e.cx[k] = (lx + hx) * HALF; e.ex[k] = (hx - lx) * HALF;
    e.cy[k] = (ly + hy) * HALF; e.ey[k] = (hy - ly) * HALF;
}

__device__ inline void load_pose_and_rects(Sight& e, const int32_t* w, const float* __restrict__ dirs, int K) {
    e.px = word_f(w, HAB_NAV2D_W_PX);
    e.py = word_f(w, HAB_NAV2D_W_PY);
    const int h = w[HAB_NAV2D_W_HEADING];
    e.c = dirs[2 * h];
    e.s = dirs[2 * h + 1];
    for (int k = 0; k < K; ++k)
        set_rect(e, k, word_f(w, HAB_NAV2D_W_RECTS + 4 * k), word_f(w, HAB_NAV2D_W_RECTS + 4 * k + 1),
                 word_f(w, HAB_NAV2D_W_RECTS + 4 * k + 2), word_f(w, HAB_NAV2D_W_RECTS + 4 * k + 3));
}

__device__ inline bool occupied(float x, float y, const Sight& e, int K) {
    for (int k = 0; k < K; ++k)
        if (x > e.x0[k] && x < e.x1[k] && y > e.y0[k] && y < e.y1[k]) return true;
    return false;
}

// The geodesic mode's `visible` on the raw rectangles: the segment agent -> (x, y) meets no open rectangle.
__device__ inline bool sees(float x, float y, const Sight& e, int K) {
    const float hx = (e.px + x) * HALF, sx = (x - e.px) * HALF;
    const float hy = (e.py + y) * HALF, sy = (y - e.py) * HALF;
    const float asx = fabsf(sx), asy = fabsf(sy);
    for (int k = 0; k < K; ++k) {
        const float mx = hx - e.cx[k], my = hy - e.cy[k];
        if (fabsf(mx) < e.ex[k] + asx && fabsf(my) < e.ey[k] + asy && fabsf(sx * my - sy * mx) < e.ex[k] * asy + e.ey[k] * asx) return false;
    }
    return true;
}

// Whether the cell with the centre (x, y) is seen from the pose: within sqrt(vis2), inside the 90 degree wedge or within 0.25 m, not
// occupied, and in sight.
__device__ inline bool seen_from(float x, float y, const Sight& e, int K, float vis2) {
    const float dx = x - e.px, dy = y - e.py;
    const float d2 = dx * dx + dy * dy;
    if (!(d2 <= vis2)) return false;
    const float dot = dx * e.c + dy * e.s, cross = e.c * dy - e.s * dx;
    return (d2 <= NEAR_R2 || (dot > 0.f && fabsf(cross) <= dot)) && !occupied(x, y, e, K) && sees(x, y, e, K);
}

}  // namespace nav2d_seen
