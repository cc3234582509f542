// Nav2D-v0: a 2-D point-goal world simulated and rendered on the device, written straight into rollout rows.
// Definition: habitat_amd/common/env_factory.py (Nav2DVectorEnv); specification: tests/nav2d_reference.py, which these
// kernels reproduce bit for bit (phi = atan2f excepted).  Every float operation below is one fp32 rounding: contraction is off
// for the whole file and division / square root are the correctly rounded forms (`__fdiv_rn` = `x / y`, `sqrt_rn` below); angles come from host-built tables.
// Nav2DVel-v0 (continuous actions) and Nav2DObj-v0 (objects, a target category, the ObjectNav sensor set) share the world, the end of
// a step and the render; their specifications are tests/nav2d_vel_reference.py and tests/nav2d_obj_reference.py.
// The geodesic distance mode of the first two tasks (nav2d_geo_build_kernel, the GEO forms of the step kernels) is specified by
// tests/nav2d_geo_reference.py, that of Nav2DObj-v0 (nav2d_obj_geo_build_kernel, nav2d_obj_geo_step_kernel: the distance to the
// nearest instance of the target category) by tests/nav2d_obj_geo_reference.py.  Nav2DRearr-v0 (one object to pick up and to put down
// at a goal that only the 1-D sensors tell) shares the world, the placement of Nav2DObj-v0 and the render; its specification is
// tests/nav2d_rearr_reference.py.  Nav2DRearrVel-v0 is that task under Nav2DVel-v0's velocity control plus a grip component; its
// specification is tests/nav2d_rearr_vel_reference.py.  The geodesic distance mode of these two (nav2d_rearr_geo_build_kernel,
// nav2d_rearr_geo_step_kernel: two fields per env, one of which moves with the object) is specified by
// tests/nav2d_rearr_geo_reference.py.  Nav2DSocial-v0 (a person who walks the graph's shortest paths, to be found and followed under
// velocity control; nav2d_social_step_kernel, nav2d_social_build_kernel) is specified by tests/nav2d_social_reference.py.
// Nav2DExplore-v0 (area coverage: the reward is the cells seen for the first time; nav2d_explore_step_kernel, one workgroup per env
// over the coverage layer, with the top-down map's rule from nav2d_seen.h) is specified by tests/nav2d_explore_reference.py.
// Nav2DImageNav-v0 (Nav2D-v0 with the goal given only as an image: nav2d_imagenav_step_kernel and the IMAGENAV form of the render, which
// draws the agent's view and the goal's in one launch) is specified by tests/nav2d_imagenav_reference.py.
// The follower (nav2d_follow_kernel) and the pick-and-place oracle (nav2d_rearr_oracle_kernel) read the geodesic fields; their
// specifications are tests/nav2d_follow_reference.py and tests/nav2d_rearr_oracle_reference.py.
// What the tasks share is written once: the moves (discrete_move, vel_decode / vel_move, on a record or on a lane's MoveLane), the
// end of a step (end_step_at for the point-goal and object tasks, rearr_end_step_at for the rearrangement tasks, close_episode under
// the latter and under the social step), the sensors' frame (to_frame), the graph of the 32-node geodesic modes (GeoGraph and its
// four helpers, which every build and every wave query goes through), the one-thread query (geo_query, on FreeBoxes) and the forward
// search over headings (forward_search).  Two places keep statements of their own because the call changes the instructions of a
// kernel that is held to them, and say so: end_step_at (close_episode's) and nav2d_rearr_step_kernel (discrete_move's).
#include <cstddef>
#include "hab_common.h"
#include "../../include/habitat_amd.h"
#include "nav2d_seen.h"

#pragma clang fp contract(off)

using namespace hab;

namespace nav2d {

__host__ __device__ inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint32_t stream_key(uint32_t seed, uint32_t sensor, uint32_t env, uint32_t t) {
    uint32_t h = mix32(seed + 0x9E3779B9u * (sensor + 1u));
    h = mix32(h ^ env);
    return mix32(h ^ t);
}
__device__ inline float u01(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }

constexpr uint32_t S_OBST = 16u, S_START = 17u, S_GOAL = 18u, S_HEAD = 19u, S_COLOR = 20u;
constexpr uint32_t S_OBJ_POS = 21u, S_OBJ_CAT = 22u, S_OBJ_TARGET = 23u;  // Nav2DObj-v0
constexpr int MAX_K = HAB_NAV2D_MAX_OBSTACLES, CANDIDATES = 16;
constexpr int MAX_M = HAB_NAV2D_MAX_OBJECTS, RING_SLOTS = 28;
constexpr float OBJ_R = 0.3f, OBJ_BLOCK = 0.4f, OBJ_LO = 0.5f, OBJ_HI = 7.5f, OBJ_APART = 1.0f, OBJ_SUCCESS = 1.0f;
constexpr float ARENA = 8.0f, RADIUS = 0.1f, LO = 0.1f, HI = 7.9f, FORWARD = 0.25f;

// One env's state (HAB_NAV2D_STATE_BYTES = 224 bytes = 56 words; the layout is part of the C ABI, see the header).
struct Nav2DState {
    float px, py, gx, gy;
    float d_prev, d_start, path;
    int32_t heading, steps, collisions, episode, ended;
    float last[4];              // success, spl, distance_to_goal, collisions of the episode that ended last
    float rect[MAX_K][4];       // x0, y0, x1, y1
    uint32_t color[MAX_K];      // r | g << 8 | b << 16
};
static_assert(sizeof(Nav2DState) == HAB_NAV2D_STATE_BYTES, "Nav2DState layout");
// the words the header names for the host side
static_assert(offsetof(Nav2DState, px) == 4 * HAB_NAV2D_W_PX && offsetof(Nav2DState, py) == 4 * HAB_NAV2D_W_PY, "Nav2DState layout");
static_assert(offsetof(Nav2DState, gx) == 4 * HAB_NAV2D_W_GX && offsetof(Nav2DState, gy) == 4 * HAB_NAV2D_W_GY, "Nav2DState layout");
static_assert(offsetof(Nav2DState, heading) == 4 * HAB_NAV2D_W_HEADING && offsetof(Nav2DState, steps) == 4 * HAB_NAV2D_W_STEPS,
              "Nav2DState layout");
static_assert(offsetof(Nav2DState, collisions) == 4 * HAB_NAV2D_W_COLLISIONS && offsetof(Nav2DState, episode) == 4 * HAB_NAV2D_W_EPISODE,
              "Nav2DState layout");
static_assert(offsetof(Nav2DState, ended) == 4 * HAB_NAV2D_W_ENDED && offsetof(Nav2DState, last) == 4 * HAB_NAV2D_W_LAST_MEASURES,
              "Nav2DState layout");
static_assert(offsetof(Nav2DState, d_prev) == 4 * HAB_NAV2D_W_D_PREV && offsetof(Nav2DState, d_start) == 4 * HAB_NAV2D_W_D_START,
              "Nav2DState layout");
static_assert(offsetof(Nav2DState, path) == 4 * HAB_NAV2D_W_PATH && offsetof(Nav2DState, rect) == 4 * HAB_NAV2D_W_RECTS, "Nav2DState layout");

// One env of Nav2DObj-v0: a Nav2D-v0 record (gx, gy = the centre of the nearest object of the target category), then the start pose
// the gps / compass sensors refer to, the target category and the objects.
struct Nav2DObjState {
    Nav2DState base;
    float sx, sy;
    int32_t h0, target;
    float obj[MAX_M][2];        // centre x, y
    int32_t cat[MAX_M];
};
static_assert(sizeof(Nav2DObjState) == HAB_NAV2D_OBJ_STATE_BYTES && offsetof(Nav2DObjState, base) == 0, "Nav2DObjState layout");
static_assert(offsetof(Nav2DObjState, sx) == 4 * HAB_NAV2D_OBJ_W_START_X && offsetof(Nav2DObjState, sy) == 4 * HAB_NAV2D_OBJ_W_START_Y,
              "Nav2DObjState layout");
static_assert(offsetof(Nav2DObjState, h0) == 4 * HAB_NAV2D_OBJ_W_START_HEADING && offsetof(Nav2DObjState, target) == 4 * HAB_NAV2D_OBJ_W_TARGET,
              "Nav2DObjState layout");
static_assert(offsetof(Nav2DObjState, obj) == 4 * HAB_NAV2D_OBJ_W_OBJECTS && offsetof(Nav2DObjState, cat) == 4 * HAB_NAV2D_OBJ_W_CATEGORIES,
              "Nav2DObjState layout");

// One env of Nav2DRearr-v0: a Nav2D-v0 record (gx, gy = the goal position, d_prev = the potential after the last step, d_start = the
// episode's first), then the agent's start and the two places of the episode in the order they are drawn (the object's start, the
// goal), named as place_positions reads them, the object's position (the agent's while it is held), the holding flag and the
// episode's counters.
struct Nav2DRearrState {
    Nav2DState base;
    float sx, sy;
    float obj[2][2];            // object start (x, y), goal (x, y)
    float ox, oy;
    int32_t holding, held, picks, invalid;
};
static_assert(sizeof(Nav2DRearrState) == HAB_NAV2D_REARR_STATE_BYTES && offsetof(Nav2DRearrState, base) == 0, "Nav2DRearrState layout");
static_assert(offsetof(Nav2DRearrState, sx) == 4 * HAB_NAV2D_REARR_W_START && offsetof(Nav2DRearrState, sy) == 4 * HAB_NAV2D_REARR_W_START + 4,
              "Nav2DRearrState layout");
static_assert(offsetof(Nav2DRearrState, obj) == 4 * HAB_NAV2D_REARR_W_OBJ_START &&
              offsetof(Nav2DRearrState, obj) + 8 == 4 * HAB_NAV2D_REARR_W_GOAL && offsetof(Nav2DRearrState, ox) == 4 * HAB_NAV2D_REARR_W_OBJ,
              "Nav2DRearrState layout");
static_assert(offsetof(Nav2DRearrState, oy) == 4 * HAB_NAV2D_REARR_W_OBJ + 4, "Nav2DRearrState layout");
static_assert(offsetof(Nav2DRearrState, holding) == 4 * HAB_NAV2D_REARR_W_HOLDING && offsetof(Nav2DRearrState, held) == 4 * HAB_NAV2D_REARR_W_HELD,
              "Nav2DRearrState layout");
static_assert(offsetof(Nav2DRearrState, picks) == 4 * HAB_NAV2D_REARR_W_PICKS && offsetof(Nav2DRearrState, invalid) == 4 * HAB_NAV2D_REARR_W_INVALID,
              "Nav2DRearrState layout");

// Correctly rounded square root.  NOT `__fsqrt_rn`: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define that name as the
// native (1 ulp) square root; `sqrtf` is the IEEE one under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt.
__device__ inline float sqrt_rn(float x) { return __builtin_sqrtf(x); }

// S: a record with the rectangles, a Nav2DState or the geodesic rearrangement step's RearrLane::Base.
template <class S>
__device__ inline bool is_free(float x, float y, const S& s, int K) {
    if (!(x >= LO && x <= HI && y >= LO && y <= HI)) return false;
    for (int k = 0; k < K; ++k)
        if (x > s.rect[k][0] - RADIUS && x < s.rect[k][2] + RADIUS && y > s.rect[k][1] - RADIUS && y < s.rect[k][3] + RADIUS)
            return false;
    return true;
}
__device__ inline float dist(float ax, float ay, float bx, float by) {
    const float dx = bx - ax, dy = by - ay;
    return sqrt_rn(dx * dx + dy * dy);
}
// The offset (dx, dy) in the frame of the heading whose direction is (c, sn): what every sensor that tells a position writes.
__device__ inline void to_frame(float dx, float dy, float c, float sn, float& dot, float& cross) {
    dot = dx * c + dy * sn;
    cross = c * dy - sn * dx;
}

// The K inflated boxes -- is_free's expressions -- computed once into registers.  is_free reads the rectangles through the state
// pointer, a memory latency per rectangle and test for the one wave that the 64 envs of a workgroup are; here the loops over k are
// unrolled over MAX_K with the uniform k < K as a guard, so every index is static and a test is straight-line compares.  The
// booleans are is_free's.
struct FreeBoxes { float x0[MAX_K], y0[MAX_K], x1[MAX_K], y1[MAX_K]; };
__device__ inline void load_free_boxes(FreeBoxes& b, const Nav2DState& s, int K) {
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
        if (k < K) {
            b.x0[k] = s.rect[k][0] - RADIUS; b.y0[k] = s.rect[k][1] - RADIUS; b.x1[k] = s.rect[k][2] + RADIUS; b.y1[k] = s.rect[k][3] + RADIUS;
        }
    }
}
__device__ inline bool is_free_boxes(float x, float y, const FreeBoxes& b, int K) {
    bool free = x >= LO && x <= HI && y >= LO && y <= HI;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k)
        if (k < K) free &= !((x > b.x0[k]) & (x < b.x1[k]) & (y > b.y0[k]) & (y < b.y1[k]));
    return free;
}

// ---- geodesic distance (distance = "geodesic" of Nav2D-v0 and Nav2DVel-v0; specification: tests/nav2d_geo_reference.py) ------------
// The field of one env's running episode (HAB_NAV2D_GEO_BYTES): D[4k + j] = the shortest-path length from corner j of obstacle k's
// inflated box to the goal over the visibility graph of those corners, +inf for a corner that is no node; whether the start reached
// the goal; the sweeps the build took; the steps of the episode at which the agent saw neither the goal nor a node.  Nav2DObj-v0's
// field (HAB_NAV2D_OBJ_GEO_BYTES) is the same layout over its 64 nodes.
constexpr int GEO_NODES = 4 * MAX_K;
constexpr float GEO_E = 0.0009765625f;  // 2^-10: what a visibility box is shrunk by
template <int NODES>
struct GeoFieldOf {
    float D[NODES];
    int32_t reachable, sweeps, lost_steps, zero[5];
};
using GeoField = GeoFieldOf<GEO_NODES>;
static_assert(sizeof(GeoField) == HAB_NAV2D_GEO_BYTES, "GeoField layout");
static_assert(offsetof(GeoField, reachable) == 4 * HAB_NAV2D_GEO_W_REACHABLE && offsetof(GeoField, sweeps) == 4 * HAB_NAV2D_GEO_W_SWEEPS &&
              offsetof(GeoField, lost_steps) == 4 * HAB_NAV2D_GEO_W_LOST_STEPS, "GeoField layout");

// Corner j of obstacle k's inflated box, in the order (X0, Y0), (X1, Y0), (X0, Y1), (X1, Y1): the expressions of is_free.
__device__ inline void geo_corner(const Nav2DState& s, int k, int j, float& x, float& y) {
    x = (j & 1) ? s.rect[k][2] + RADIUS : s.rect[k][0] - RADIUS;
    y = (j & 2) ? s.rect[k][3] + RADIUS : s.rect[k][1] - RADIUS;
}
// A visibility box as centre and half extent per axis: the inflated box (x0, y0) .. (x1, y1) shrunk by GEO_E; and obstacle k's.
struct GeoBox { float cx, ex, cy, ey; };
__device__ inline GeoBox geo_box(float x0, float y0, float x1, float y1) {
    const float lx = x0 + GEO_E, ly = y0 + GEO_E;
    const float hx = x1 - GEO_E, hy = y1 - GEO_E;
    return GeoBox{(lx + hx) * 0.5f, (hx - lx) * 0.5f, (ly + hy) * 0.5f, (hy - ly) * 0.5f};
}
__device__ inline GeoBox geo_box(const Nav2DState& s, int k) {
    return geo_box(s.rect[k][0] - RADIUS, s.rect[k][1] - RADIUS, s.rect[k][2] + RADIUS, s.rect[k][3] + RADIUS);
}
// Whether the segment a-b meets the open box: the separating-axis test.
__device__ inline bool geo_blocked(const GeoBox& b, float ax, float ay, float bx, float by) {
    const float mx = (ax + bx) * 0.5f - b.cx, sx = (bx - ax) * 0.5f;
    const float my = (ay + by) * 0.5f - b.cy, sy = (by - ay) * 0.5f;
    return fabsf(mx) < b.ex + fabsf(sx) && fabsf(my) < b.ey + fabsf(sy) &&
           fabsf(sx * my - sy * mx) < b.ex * fabsf(sy) + b.ey * fabsf(sx);
}
// Whether a-b misses all K boxes; `boxes` is the build kernel's LDS array.
__device__ inline bool geo_visible(const GeoBox* boxes, int K, float ax, float ay, float bx, float by) {
    for (int k = 0; k < K; ++k)
        if (geo_blocked(boxes[k], ax, ay, bx, by)) return false;
    return true;
}
// geo(p) of one env by one thread: the goal if p sees it, and the nodes p sees, each with its field value.  The K inflated boxes
// (FreeBoxes) and visibility boxes are computed once into registers, so a visibility test is straight-line arithmetic over the boxes
// with no load and no branch in it.
// p = (px, py) is the point the distance is taken from: the agent's position for the step kernels, a candidate's target for the
// follower.  T = (tx, ty) is the target and D[GEO_NODES] the field towards it: the record's goal and GeoField::D for Nav2D-v0 and
// Nav2DVel-v0, the goal with DG or the object's place with DO for the rearrangement oracle.
__device__ inline float geo_query(const Nav2DState& s, const float* __restrict__ D, int K, float px, float py, float tx, float ty) {
    FreeBoxes corner;
    load_free_boxes(corner, s, K);
    GeoBox box[MAX_K];
#pragma unroll
    for (int k = 0; k < MAX_K; ++k)
        if (k < K) box[k] = geo_box(corner.x0[k], corner.y0[k], corner.x1[k], corner.y1[k]);
    auto sees = [&](float x, float y) {
        bool blocked = false;
#pragma unroll
        for (int k = 0; k < MAX_K; ++k)
            if (k < K) blocked |= geo_blocked(box[k], px, py, x, y);
        return !blocked;
    };
    float best = sees(tx, ty) ? dist(px, py, tx, ty) : INFINITY;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
        if (k < K) {
            const float x0 = corner.x0[k], y0 = corner.y0[k], x1 = corner.x1[k], y1 = corner.y1[k];
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const float Di = D[4 * k + j];
                if (!(Di < INFINITY)) continue;
                const float x = (j & 1) ? x1 : x0, y = (j & 2) ? y1 : y0;
                if (sees(x, y)) best = fminf(best, dist(px, py, x, y) + Di);
            }
        }
    }
    return best;
}

// What one wavefront keeps in LDS of one env's graph: the 32 nodes, the K visibility boxes, the symmetric 32 x 32 weight matrix
// (4 KiB) and two copies of D.  The nodes and boxes serve the queries; the weights and the two copies of D a build.
struct GeoGraph {
    float node_x[GEO_NODES], node_y[GEO_NODES];
    int node_ok[GEO_NODES];
    GeoBox boxes[MAX_K];
    float W[GEO_NODES * GEO_NODES];
    float D[2][GEO_NODES];
};
// The nodes (lane l < 32: node l), the diagonal of the weights and the K visibility boxes (lanes 32 ..); the caller puts the barrier
// after it.
__device__ inline void geo_graph_nodes(GeoGraph& G, const Nav2DState& s, int K, int lane) {
    if (lane < GEO_NODES) {
        float x = 0.0f, y = 0.0f;
        bool ok = false;
        if (lane < 4 * K) {
            geo_corner(s, lane >> 2, lane & 3, x, y);
            ok = is_free(x, y, s, K);
        }
        G.node_x[lane] = x; G.node_y[lane] = y; G.node_ok[lane] = ok ? 1 : 0;
        G.W[lane * GEO_NODES + lane] = INFINITY;
    } else if (lane - GEO_NODES < K) {
        G.boxes[lane - GEO_NODES] = geo_box(s, lane - GEO_NODES);
    }
}
// The symmetric weights; needs the nodes, and a barrier after it.  The 496 node pairs go round the lanes, 8 rounds: pair p lies in
// rows a and 30 - a, which hold 32 pairs together (row 15 alone 16).
__device__ inline void geo_graph_weights(GeoGraph& G, int K, int lane) {
    for (int p = lane; p < GEO_NODES * (GEO_NODES - 1) / 2; p += 64) {
        const int a = p >> 5, c = p & 31;
        const int i = c < 31 - a ? a : 30 - a;
        const int j = c < 31 - a ? a + 1 + c : i + 1 + (c - (31 - a));
        float w = INFINITY;
        if (G.node_ok[i] && G.node_ok[j] && geo_visible(G.boxes, K, G.node_x[i], G.node_y[i], G.node_x[j], G.node_y[j]))
            w = dist(G.node_x[i], G.node_y[i], G.node_x[j], G.node_y[j]);
        G.W[i * GEO_NODES + j] = w;
        G.W[j * GEO_NODES + i] = w;
    }
}
// One field by one wavefront, towards the target (tx, ty), over a graph whose nodes and weights are in LDS behind a barrier.  The 32
// last hops take one lane each.  For the sweeps lane l owns half h = l & 1 of row i = l >> 1, its 16 weights in registers (read as
// column i of rows 16 h + t: 32 banks, the two halves 2-way); a sweep reads D from one copy, joins the two halves of a row with one
// lane exchange and writes the other copy, and the wave votes on whether any row changed.  Returns the sweeps; `Dl` is D[lane] on the
// lanes below 32 and +inf on the others.  Uniform over the wave; ends behind a barrier, so that another field may follow.
__device__ inline int geo_field_towards(GeoGraph& G, int K, float tx, float ty, int lane, float& Dl) {
    if (lane < GEO_NODES) {
        float d = INFINITY;
        if (G.node_ok[lane] && geo_visible(G.boxes, K, G.node_x[lane], G.node_y[lane], tx, ty)) d = dist(G.node_x[lane], G.node_y[lane], tx, ty);
        G.D[0][lane] = d;
    }
    __syncthreads();
    const int row = lane >> 1, half = lane & 1;
    float w[GEO_NODES / 2];
#pragma unroll
    for (int t = 0; t < GEO_NODES / 2; ++t) w[t] = G.W[(half * (GEO_NODES / 2) + t) * GEO_NODES + row];
    int cur = 0, sweeps = 0;
    while (sweeps < 4 * K) {  // the loop is uniform over the wave: K is an argument, the exit a vote
        sweeps += 1;
        float m = INFINITY;
#pragma unroll
        for (int t = 0; t < GEO_NODES / 2; ++t) m = fminf(m, w[t] + G.D[cur][half * (GEO_NODES / 2) + t]);
        m = fminf(m, __shfl_xor(m, 1));
        const float before = G.D[cur][row];
        const float after = fminf(before, m);
        if (half == 0) G.D[cur ^ 1][row] = after;
        const bool changed = __ballot(after != before) != 0;
        __syncthreads();
        cur ^= 1;
        if (!changed) break;
    }
    Dl = lane < GEO_NODES ? G.D[cur][lane] : INFINITY;
    __syncthreads();
    return sweeps;
}
// geo_T(x) by one wavefront: node l with its field value Dl on lane l < 32, the direct hop to the target T on lane 32, then the
// minimum over the wave, which is exact and so the same as geo_query's serial one.  Needs the nodes and boxes in LDS.
__device__ inline float geo_query_wave(const GeoGraph& G, int K, float x, float y, float tx, float ty, float Dl, int lane) {
    float v = INFINITY;
    if (lane < GEO_NODES) {
        if (Dl < INFINITY && geo_visible(G.boxes, K, x, y, G.node_x[lane], G.node_y[lane])) v = dist(x, y, G.node_x[lane], G.node_y[lane]) + Dl;
    } else if (lane == GEO_NODES) {
        if (geo_visible(G.boxes, K, x, y, tx, ty)) v = dist(x, y, tx, ty);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// The field of one env per 64-thread workgroup (one wavefront).  Selected are the envs whose `mask` byte is set (NULL: all) and, with
// `only_ended`, whose last step ended an episode; every other workgroup leaves before the first barrier.  The graph, the field towards
// the goal, then g0 = geo(current position), which becomes the episode's first distance where it is finite.
__global__ void __launch_bounds__(64)
nav2d_geo_build_kernel(char* __restrict__ states, size_t state_stride, GeoField* __restrict__ geo, const uint8_t* __restrict__ mask,
                       int only_ended, int K) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    Nav2DState& s = *reinterpret_cast<Nav2DState*>(states + (size_t)n * state_stride);
    if (only_ended && !s.ended) return;
    __shared__ GeoGraph G;
    geo_graph_nodes(G, s, K, lane);
    __syncthreads();
    geo_graph_weights(G, K, lane);
    const float px = s.px, py = s.py, gx = s.gx, gy = s.gy;
    __syncthreads();
    float Dl;
    const int sweeps = geo_field_towards(G, K, gx, gy, lane, Dl);
    if (lane < GEO_NODES) geo[n].D[lane] = Dl;
    const float v = geo_query_wave(G, K, px, py, gx, gy, Dl, lane);
    if (lane == 0) {
        const bool reachable = v < INFINITY;
        geo[n].reachable = reachable ? 1 : 0;
        geo[n].sweeps = sweeps;
        geo[n].lost_steps = 0;
        for (int z = 0; z < 5; ++z) geo[n].zero[z] = 0;
        if (reachable) s.d_start = s.d_prev = v;
    }
}

// A new episode's world.  GOAL (Nav2D-v0, Nav2DVel-v0): rectangles, their colours, the start, the goal, the heading, the distances and
// the counters.  Without GOAL (Nav2DObj-v0) the goal and the distances are left to the caller, which places its objects afterwards.
template <bool GOAL = true>
__device__ void begin_episode(Nav2DState& s, uint32_t seed, uint32_t env, int K, int nh) {
    const uint32_t ep = (uint32_t)s.episode;
    const uint32_t ko = stream_key(seed, S_OBST, env, ep), kc = stream_key(seed, S_COLOR, env, ep);
    for (int k = 0; k < K; ++k) {
        const float cx = 2.0f + 4.0f * u01(mix32(ko ^ (uint32_t)(4 * k))), cy = 2.0f + 4.0f * u01(mix32(ko ^ (uint32_t)(4 * k + 1)));
        const float hx = 0.25f + 0.75f * u01(mix32(ko ^ (uint32_t)(4 * k + 2))), hy = 0.25f + 0.75f * u01(mix32(ko ^ (uint32_t)(4 * k + 3)));
        s.rect[k][0] = cx - hx; s.rect[k][1] = cy - hy; s.rect[k][2] = cx + hx; s.rect[k][3] = cy + hy;
        const uint32_t c = mix32(kc ^ (uint32_t)k);
        s.color[k] = (64u + (c & 127u)) | ((64u + ((c >> 8) & 127u)) << 8) | ((64u + ((c >> 16) & 127u)) << 16);
    }
    const uint32_t ks = stream_key(seed, S_START, env, ep), kg = stream_key(seed, S_GOAL, env, ep);
    float sx = 0.5f, sy = 0.5f;
    for (int j = 0; j < CANDIDATES; ++j) {
        const float x = LO + 7.8f * u01(mix32(ks ^ (uint32_t)(2 * j))), y = LO + 7.8f * u01(mix32(ks ^ (uint32_t)(2 * j + 1)));
        if (is_free(x, y, s, K)) { sx = x; sy = y; break; }
    }
    float gx = 7.5f, gy = 7.5f;
    if constexpr (GOAL) {
        for (int j = 0; j < CANDIDATES; ++j) {
            const float x = LO + 7.8f * u01(mix32(kg ^ (uint32_t)(2 * j))), y = LO + 7.8f * u01(mix32(kg ^ (uint32_t)(2 * j + 1)));
            if (is_free(x, y, s, K) && dist(sx, sy, x, y) >= 1.0f) { gx = x; gy = y; break; }
        }
    }
    s.px = sx; s.py = sy;
    if constexpr (GOAL) { s.gx = gx; s.gy = gy; }
    s.heading = (int32_t)(mix32(stream_key(seed, S_HEAD, env, ep) ^ 0u) % (uint32_t)nh);
    if constexpr (GOAL) s.d_start = s.d_prev = dist(sx, sy, gx, gy);
    s.path = 0.0f;
    s.steps = 0;
    s.collisions = 0;
}

// Episode 0 of one env (advance = 0 of every step kernel; GOAL as in begin_episode).
template <bool GOAL = true>
__device__ inline void first_episode(Nav2DState& s, uint32_t seed, uint32_t env, int K, int nh) {
    s.episode = 0;
    s.ended = 0;
    s.last[0] = s.last[1] = s.last[2] = s.last[3] = 0.0f;
    begin_episode<GOAL>(s, seed, env, K, nh);
}

// What ends an episode in every task: the four measures of the episode, their sums, and the next episode's world
// (`begin_episode<GOAL>`; a task with more than a world then adds its own where `ended` is set or right after this).
template <bool GOAL>
__device__ inline void close_episode(Nav2DState& s, float m0, float m1, float m2, float m3, float* __restrict__ sums, uint32_t seed,
                                     uint32_t env, int n, int N, int K, int nh) {
    s.last[0] = m0;
    s.last[1] = m1;
    s.last[2] = m2;
    s.last[3] = m3;
    if (sums)
        for (int m = 0; m < 4; ++m) sums[(size_t)m * N + n] = sums[(size_t)m * N + n] + s.last[m];
    s.episode += 1;
    begin_episode<GOAL>(s, seed, env, K, nh);
}

// What follows the move of one step of the point-goal and object tasks, given the distance `d` of the new position: reward, step
// count, done, and on done the measures, their sums and the next episode's world (the object task then adds its objects where
// `ended` is set).  `stop` is the action's request to end the episode (STOP / both speeds below their minima), `success_dist` the
// task's success radius.  The statements of close_episode are written out here and not called: with the call, the Nav2D-v0,
// Nav2DVel-v0 and Nav2DObj-v0 step kernels are no longer the instructions they were, and two earlier forms of sharing in this
// function (the distance computed by the kernel and the next world begun by it; the next world as a callable) compiled to a velocity
// kernel whose distance was that of the previous position.  Whoever changes this function compares those kernels' code.
template <bool GOAL>
__device__ inline void end_step_at(Nav2DState& s, float d, bool stop, float success_dist, float* __restrict__ reward,
                                   uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed, uint32_t env, int n, int N,
                                   int K, int nh, int max_steps) {
    const bool success = stop && (d < success_dist);
    reward[n] = (-0.01f + (s.d_prev - d)) + (success ? 2.5f : 0.0f);
    s.d_prev = d;
    s.steps += 1;
    const bool done = stop || (s.steps >= max_steps);
    not_done[n] = done ? 0 : 1;
    s.ended = done ? 1 : 0;
    if (done) {
        s.last[0] = success ? 1.0f : 0.0f;
        s.last[1] = success ? __fdiv_rn(s.d_start, fmaxf(s.d_start, s.path)) : 0.0f;
        s.last[2] = d;
        s.last[3] = (float)s.collisions;
        if (sums)
            for (int m = 0; m < 4; ++m) sums[(size_t)m * N + n] = sums[(size_t)m * N + n] + s.last[m];
        s.episode += 1;
        begin_episode<GOAL>(s, seed, env, K, nh);
    }
}
// The distance to (gx, gy) of the new position, then end_step_at.  GEO: `geo` is the env's field; in a reachable episode the
// distance is geo(p), and d_prev where p sees nothing (a lost step).
template <bool GOAL = true, bool GEO = false>
__device__ inline void end_step(Nav2DState& s, bool stop, float success_dist, float* __restrict__ reward, uint8_t* __restrict__ not_done,
                                float* __restrict__ sums, uint32_t seed, uint32_t env, int n, int N, int K, int nh, int max_steps,
                                GeoField* geo = nullptr) {
    float d = dist(s.px, s.py, s.gx, s.gy);
    if constexpr (GEO) {
        if (geo->reachable) {
            d = geo_query(s, geo->D, K, s.px, s.py, s.gx, s.gy);
            if (!(d < INFINITY)) { d = s.d_prev; geo->lost_steps += 1; }
        }
    }
    end_step_at<GOAL>(s, d, stop, success_dist, reward, not_done, sums, seed, env, n, N, K, nh, max_steps);
}

// The move of a discrete action: FORWARD under the task's free test `free(x, y)`, TURN_LEFT, TURN_RIGHT; every other action moves
// nothing.  S: a record, or a lane's copy of the words a move changes.
template <class S, class Free>
__device__ inline void discrete_move(S& s, int64_t a, const float* __restrict__ dirs, int nh, Free free) {
    if (a == 1) {
        const float nx = s.px + FORWARD * dirs[2 * s.heading], ny = s.py + FORWARD * dirs[2 * s.heading + 1];
        if (free(nx, ny)) { s.px = nx; s.py = ny; s.path = s.path + FORWARD; }
        else s.collisions += 1;
    } else if (a == 2) {
        s.heading = (s.heading + 1) % nh;
    } else if (a == 3) {
        s.heading = (s.heading + nh - 1) % nh;
    }
}

// pointgoal_with_gps_compass of the current state.
__device__ inline void write_goal(const Nav2DState& s, const float* __restrict__ dirs, float* __restrict__ goal, int n) {
    const float c = dirs[2 * s.heading], sn = dirs[2 * s.heading + 1];
    float dot, cross;
    to_frame(s.gx - s.px, s.gy - s.py, c, sn, dot, cross);
    goal[2 * n + 0] = dist(s.px, s.py, s.gx, s.gy);
    goal[2 * n + 1] = atan2f(cross, dot);
}

// One thread per env.  advance = 0: episode 0 of every selected env; advance = 1: one step with actions[n].  Then the goal sensor.
// GEO: launched with 64 threads a workgroup, and told so: the query keeps the boxes of the world in registers.
template <bool GEO>
__global__ void __launch_bounds__(GEO ? 64 : 1024) nav2d_step_kernel(Nav2DState* __restrict__ states, const float* __restrict__ dirs, const int64_t* __restrict__ actions,
                                  const uint8_t* __restrict__ mask, float* __restrict__ goal, float* __restrict__ reward,
                                  uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed, uint32_t env_offset, int N,
                                  int K, int nh, int max_steps, int advance, GeoField* __restrict__ geo) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (mask && !mask[n])) return;
    Nav2DState& s = states[n];  // worked on in place: a private copy indexed by k would live in scratch memory
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        first_episode(s, seed, env, K, nh);
    } else {
        const int64_t a = actions[n];  // anything outside 0..3 moves nothing (the host-side entry points refuse it)
        discrete_move(s, a, dirs, nh, [&](float x, float y) { return is_free(x, y, s, K); });
        end_step<true, GEO>(s, a == 0, 0.2f, reward, not_done, sums, seed, env, n, N, K, nh, max_steps, GEO ? geo + n : nullptr);
    }
    if (goal) write_goal(s, dirs, goal, n);
}

// Nav2DVel-v0 (Nav2DVelVectorEnv; specification: tests/nav2d_vel_reference.py): the same record, world, reward, measures and sensors,
// with a continuous action (a_lin, a_ang), one 8-byte row of an (N, 2) float32 tensor.  Each component is clamped to [-1, 1], a
// non-finite one acts as 0; the step length is (c_lin + 1) * 0.125, the turn rint(c_ang * max_turn) heading quanta (left positive),
// and both below their minima is the stop.  A blocked target counts one collision and, with sliding, the agent takes the x or else
// the y component of the move alone where that is free.  The heading stays an index into `dirs`: no angle is evaluated here.
// The three helpers are the velocity control of Nav2DVel-v0 and Nav2DRearrVel-v0 alike.
__device__ inline float vel_clamp(float a) { return isfinite(a) ? fminf(fmaxf(a, -1.0f), 1.0f) : 0.0f; }
// Steps 1-4: the step length and the turn of (a_lin, a_ang); returns the stop.
__device__ inline bool vel_decode(float a_lin, float a_ang, int max_turn, int stop_turn, float min_lin, float& l, int& dh) {
    const float c_lin = vel_clamp(a_lin), c_ang = vel_clamp(a_ang);
    l = (c_lin + 1.0f) * 0.125f;
    dh = (int)rintf(c_ang * (float)max_turn);  // |dh| <= max_turn <= nh / 2
    return (l < min_lin) && (abs(dh) < stop_turn);
}
// Step 5: the turn, then the move of length l under the task's free test `free(x, y)`.
template <class S, class Free>
__device__ inline void vel_move(S& s, const float* __restrict__ dirs, float l, int dh, int nh, int sliding, Free free) {
    s.heading = (s.heading + dh + nh) % nh;
    const float nx = s.px + l * dirs[2 * s.heading], ny = s.py + l * dirs[2 * s.heading + 1];
    if (free(nx, ny)) {
        s.px = nx; s.py = ny; s.path = s.path + l;
    } else {
        s.collisions += 1;
        if (sliding) {
            if (free(nx, s.py)) { s.path = s.path + fabsf(nx - s.px); s.px = nx; }
            else if (free(s.px, ny)) { s.path = s.path + fabsf(ny - s.py); s.py = ny; }
        }
    }
}
// What a move changes of a record, as a lane's own copy in registers: the members discrete_move and vel_move read and write.  In a
// kernel of one wavefront per env every lane derives the move on its copy, from the same loads, and lane 0 writes it back.
struct MoveLane {
    float px, py, path;
    int32_t heading, collisions;
};
__device__ inline MoveLane load_move(const Nav2DState& s) { return MoveLane{s.px, s.py, s.path, s.heading, s.collisions}; }
template <class L>
__device__ inline void store_move(Nav2DState& s, const L& m) {
    s.px = m.px; s.py = m.py; s.path = m.path; s.heading = m.heading; s.collisions = m.collisions;
}

template <bool GEO>
__global__ void __launch_bounds__(GEO ? 64 : 1024) nav2d_vel_step_kernel(Nav2DState* __restrict__ states, const float* __restrict__ dirs, const float2* __restrict__ actions,
                                      const uint8_t* __restrict__ mask, float* __restrict__ goal, float* __restrict__ reward,
                                      uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed, uint32_t env_offset,
                                      int N, int K, int nh, int max_steps, int max_turn, int stop_turn, float min_lin, int sliding,
                                      int advance, GeoField* __restrict__ geo) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (mask && !mask[n])) return;
    Nav2DState& s = states[n];
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        first_episode(s, seed, env, K, nh);
    } else {
        const float2 a = actions[n];
        float l;
        int dh;
        const bool stop = vel_decode(a.x, a.y, max_turn, stop_turn, min_lin, l, dh);
        if (!stop) vel_move(s, dirs, l, dh, nh, sliding, [&](float x, float y) { return is_free(x, y, s, K); });
        end_step<true, GEO>(s, stop, 0.2f, reward, not_done, sums, seed, env, n, N, K, nh, max_steps, GEO ? geo + n : nullptr);
    }
    if (goal) write_goal(s, dirs, goal, n);
}

// ---- the shortest-path follower of Nav2D-v0 and Nav2DVel-v0 (specification: tests/nav2d_follow_reference.py) -----------------------
// What turns the rule's answer into the task's action.  `go` is status GO, `delta` the signed number of heading quanta to the winner.
struct FollowDiscrete {
    using Action = int64_t;
    __device__ Action operator()(bool go, int delta) const { return !go ? 0 : delta == 0 ? 1 : delta > 0 ? 2 : 3; }
};
struct FollowVelocity {
    using Action = float2;
    int max_turn;
    __device__ Action operator()(bool go, int delta) const {
        if (!go) return make_float2(-1.0f, 0.0f);
        if (abs(delta) <= max_turn) return make_float2(1.0f, __fdiv_rn((float)delta, (float)max_turn));  // decodes to l = 0.25, dh = delta
        return make_float2(-1.0f, delta > 0 ? 1.0f : -1.0f);                                             // a turn in place of max_turn
    }
};

// The turns from `heading` to h as a key that orders like (|delta|, delta < 0): delta = (h - heading) mod nh, minus nh where
// 2 * delta > nh, so the half turn stays positive (left); and the delta of such a key.
__device__ inline uint32_t turn_key(int h, int heading, int nh) {
    int d = (h - heading) % nh;
    if (d < 0) d += nh;
    if (2 * d > nh) d -= nh;
    return ((uint32_t)abs(d) << 1) | (d < 0 ? 1u : 0u);
}
__device__ inline int turn_key_delta(uint32_t k) {
    const int turns = (int)(k >> 1);
    return (k & 1u) ? -turns : turns;
}
// The least of the wave's 64-bit keys, on every lane.
__device__ inline unsigned long long wave_min_key(unsigned long long key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    return key;
}

// The forward search of the follower and of the oracle, by one wavefront: lane = candidate heading, the lanes stride over the nh
// headings by 64.  A lane's candidate is the target p' of a forward at its heading; where p' is free under the task's test
// `free(x, y)` it runs the straight-line query of the step kernels at p', towards T = (tx, ty) over the field D.  A valid candidate
// (v finite and below `bound`) has the 64-bit key v's bits << 32 | |delta| << 1 | (delta < 0): v is not negative, so the bit patterns
// order like the floats, and the least key is the lowest value, then the fewest turns, then left.  Returns the least key of the
// wave, NO_KEY where no candidate is valid.  Everything but `lane` is uniform over the wave.
constexpr unsigned long long NO_KEY = ~0ull;
template <class Free>
__device__ inline unsigned long long forward_search(const Nav2DState& s, const float* __restrict__ D, const float* __restrict__ dirs, int K,
                                                    int nh, float tx, float ty, float bound, int lane, Free free) {
    const float px = s.px, py = s.py;
    const int heading = s.heading;
    unsigned long long key = NO_KEY;
    for (int h0 = 0; h0 < nh; h0 += 64) {  // uniform over the wave
        const int h = h0 + lane;
        if (h >= nh) continue;
        const float nx = px + FORWARD * dirs[2 * h], ny = py + FORWARD * dirs[2 * h + 1];
        if (!free(nx, ny)) continue;
        const float v = geo_query(s, D, K, nx, ny, tx, ty);
        if (!(v < INFINITY && v < bound)) continue;
        const unsigned long long k = ((unsigned long long)__float_as_uint(v) << 32) | turn_key(h, heading, nh);
        key = k < key ? k : key;
    }
    return wave_min_key(key);
}

// One env per 64-thread workgroup (one wavefront), selected by `mask` (NULL: all).  State and field are read only, through pointers
// that are uniform over the wave.  The forward search towards the goal below D_PREV; lane 0 writes the action, next_d and status.
template <class Writer>
__global__ void __launch_bounds__(64)
nav2d_follow_kernel(const char* __restrict__ states, size_t state_stride, const GeoField* __restrict__ geo, const float* __restrict__ dirs,
                    const uint8_t* __restrict__ mask, typename Writer::Action* __restrict__ actions, float* __restrict__ next_d,
                    int32_t* __restrict__ status, int K, int nh, Writer writer) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    const Nav2DState& s = *reinterpret_cast<const Nav2DState*>(states + (size_t)n * state_stride);
    const GeoField& g = geo[n];
    const float d_prev = s.d_prev;
    int st, delta = 0;
    float nd = INFINITY;
    if (!g.reachable) {
        st = HAB_NAV2D_FOLLOW_UNREACHABLE;
    } else if (d_prev < 0.2f) {
        st = HAB_NAV2D_FOLLOW_ARRIVED;
        nd = d_prev;
    } else {
        const unsigned long long key =
            forward_search(s, g.D, dirs, K, nh, s.gx, s.gy, d_prev, lane, [&](float x, float y) { return is_free(x, y, s, K); });
        if (key == NO_KEY) {
            st = HAB_NAV2D_FOLLOW_STUCK;
        } else {
            st = HAB_NAV2D_FOLLOW_GO;
            nd = __uint_as_float((uint32_t)(key >> 32));
            delta = turn_key_delta((uint32_t)key);
        }
    }
    if (lane == 0) {
        actions[n] = writer(st == HAB_NAV2D_FOLLOW_GO, delta);
        if (next_d) next_d[n] = nd;
        if (status) status[n] = st;
    }
}

// ---- Nav2DObj-v0 (Nav2DObjVectorEnv; specification: tests/nav2d_obj_reference.py) -----------------------------------------------------
__device__ inline bool is_free_obj(float x, float y, const Nav2DObjState& s, int K, int M) {
    if (!is_free(x, y, s.base, K)) return false;
    for (int j = 0; j < M; ++j)
        if (dist(x, y, s.obj[j][0], s.obj[j][1]) < OBJ_BLOCK) return false;
    return true;
}
// Whether (x, y) can take object j: clear of the start and of the objects before it.  S: a record with the start (sx, sy) and obj.
template <class S>
__device__ inline bool object_fits(float x, float y, const S& s, int j) {
    if (!(dist(s.sx, s.sy, x, y) >= OBJ_APART)) return false;
    for (int i = 0; i < j; ++i)
        if (!(dist(s.obj[i][0], s.obj[i][1], x, y) >= OBJ_APART)) return false;
    return true;
}
// Slot q of the fallback ring: the 28 points one metre apart on the square through (0.5, 0.5) and (7.5, 7.5), counter-clockwise
// from (0.5, 0.5).  No rectangle grown by 0.3 reaches them.
__device__ inline void ring_slot(int q, float& x, float& y) {
    const int side = q / 7;
    const float i = (float)(q - 7 * side);
    x = side == 0 ? 0.5f + i : side == 1 ? 7.5f : side == 2 ? 7.5f - i : 0.5f;
    y = side == 0 ? 0.5f : side == 1 ? 0.5f + i : side == 2 ? 7.5f : 7.5f - i;
}
// The nearest centre of the target category becomes (gx, gy); returns its distance.  The first of equally near ones wins.
__device__ inline float nearest_target(Nav2DObjState& s, int M) {
    float best = INFINITY;
    for (int j = 0; j < M; ++j) {
        if (s.cat[j] != s.target) continue;
        const float d = dist(s.base.px, s.base.py, s.obj[j][0], s.obj[j][1]);
        if (d < best) { best = d; s.base.gx = s.obj[j][0]; s.base.gy = s.obj[j][1]; }
    }
    return best;
}
// Whether (x, y) lies strictly inside one of the K rectangles grown by the object radius.
template <class S>
__device__ inline bool in_grown_rect(float x, float y, const S& s, int K) {
    bool in_rect = false;
    for (int k = 0; k < K; ++k)
        in_rect = in_rect || (x > s.rect[k][0] - OBJ_R && x < s.rect[k][2] + OBJ_R && y > s.rect[k][1] - OBJ_R && y < s.rect[k][3] + OBJ_R);
    return in_rect;
}
// The positions of M objects in the world of `s.base`, whose start (sx, sy) the record holds.  `kp` is the key of stream 21 of the
// episode, which gives the 16 candidates of each object; then the ring.  `each(j)` runs once object j has its place.  Nav2DObj-v0's
// objects, and with M = 2 Nav2DRearr-v0's object start and goal.
template <class S, class Each>
__device__ inline void place_positions(S& s, uint32_t kp, int K, int M, Each each) {
    for (int j = 0; j < M; ++j) {
        bool placed = false;
        for (int i = 0; i < CANDIDATES && !placed; ++i) {
            const uint32_t w = (uint32_t)(2 * (CANDIDATES * j + i));
            const float x = LO + 7.8f * u01(mix32(kp ^ w)), y = LO + 7.8f * u01(mix32(kp ^ (w + 1u)));
            if (!(x >= OBJ_LO && x <= OBJ_HI && y >= OBJ_LO && y <= OBJ_HI)) continue;
            if (in_grown_rect(x, y, s.base, K) || !object_fits(x, y, s, j)) continue;
            s.obj[j][0] = x; s.obj[j][1] = y;
            placed = true;
        }
        for (int q = 0; q < RING_SLOTS && !placed; ++q) {  // a fitting slot always exists, see the restatement
            float x, y;
            ring_slot(q, x, y);
            s.obj[j][0] = x; s.obj[j][1] = y;
            placed = object_fits(x, y, s, j);
        }
        each(j);
    }
}
// What Nav2DObj-v0 adds to a world that `begin_episode<false>` has just generated: the start pose the gps / compass sensors refer to,
// the objects, the target, and the distances.
__device__ void place_objects(Nav2DObjState& s, uint32_t seed, uint32_t env, int K, int M, int C) {
    const uint32_t ep = (uint32_t)s.base.episode;
    s.sx = s.base.px; s.sy = s.base.py; s.h0 = s.base.heading;
    const uint32_t kp = stream_key(seed, S_OBJ_POS, env, ep), kc = stream_key(seed, S_OBJ_CAT, env, ep);
    place_positions(s, kp, K, M, [&](int j) { s.cat[j] = (int32_t)(mix32(kc ^ (uint32_t)j) % (uint32_t)C); });
    for (int j = M; j < MAX_M; ++j) { s.obj[j][0] = 0.0f; s.obj[j][1] = 0.0f; s.cat[j] = -1; }
    s.target = s.cat[mix32(stream_key(seed, S_OBJ_TARGET, env, ep) ^ 0u) % (uint32_t)M];
    s.base.d_start = s.base.d_prev = nearest_target(s, M);
}

// The three 1-D sensors: objectgoal, gps (the offset from the start in the start heading's frame) and compass (a row of the host
// table).
__device__ inline void obj_write_sensors(const Nav2DObjState& o, const float* __restrict__ dirs, const float* __restrict__ ctab,
                                         int64_t* __restrict__ objectgoal, float* __restrict__ gps, float* __restrict__ compass, int n, int nh) {
    const Nav2DState& s = o.base;
    if (objectgoal) objectgoal[n] = (int64_t)o.target;
    if (gps) {
        const float c = dirs[2 * o.h0], sn = dirs[2 * o.h0 + 1];
        to_frame(s.px - o.sx, s.py - o.sy, c, sn, gps[2 * n + 0], gps[2 * n + 1]);
    }
    if (compass) compass[n] = ctab[(s.heading - o.h0 + nh) % nh];
}

// One thread per env, as nav2d_step_kernel.  Then the sensors.
__global__ void nav2d_obj_step_kernel(Nav2DObjState* __restrict__ states, const float* __restrict__ dirs, const float* __restrict__ ctab,
                                      const int64_t* __restrict__ actions, const uint8_t* __restrict__ mask,
                                      int64_t* __restrict__ objectgoal, float* __restrict__ gps, float* __restrict__ compass,
                                      float* __restrict__ reward, uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed,
                                      uint32_t env_offset, int N, int K, int nh, int max_steps, int M, int C, int advance) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (mask && !mask[n])) return;
    Nav2DObjState& o = states[n];
    Nav2DState& s = o.base;
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        first_episode<false>(s, seed, env, K, nh);
        place_objects(o, seed, env, K, M, C);
    } else {
        const int64_t a = actions[n];  // 4, 5 (LOOK_UP, LOOK_DOWN) and anything outside 0..5 move nothing
        discrete_move(s, a, dirs, nh, [&](float x, float y) { return is_free_obj(x, y, o, K, M); });
        nearest_target(o, M);  // (gx, gy) of this step, which end_step measures the distance to
        end_step<false>(s, a == 0, OBJ_SUCCESS, reward, not_done, sums, seed, env, n, N, K, nh, max_steps);
        if (s.ended) place_objects(o, seed, env, K, M, C);
    }
    obj_write_sensors(o, dirs, ctab, objectgoal, gps, compass, n, nh);
}

// ---- Nav2DRearr-v0 (Nav2DRearrVectorEnv; specification: tests/nav2d_rearr_reference.py) ------------------------------------------------
constexpr float REARR_REACH = 1.0f, REARR_ARM = 0.5f, REARR_SUCCESS = 0.5f;

// The potential d(p, o) + d(o, g) of the current state; `b` is its second term.  A held object is at p, so the first term is 0.
__device__ inline float rearr_potential(const Nav2DRearrState& r, float& b) {
    const Nav2DState& s = r.base;
    b = dist(r.ox, r.oy, s.gx, s.gy);
    return dist(s.px, s.py, r.ox, r.oy) + b;
}
// What Nav2DRearr-v0 adds to a world that `begin_episode<false>` has just generated: the two places (Nav2DObj-v0's objects 0 and 1 of
// that world), the object at its start or in the agent's hand, the counters and the first potential.
__device__ inline void rearr_begin(Nav2DRearrState& r, uint32_t seed, uint32_t env, int K, int start_holding) {
    Nav2DState& s = r.base;
    r.sx = s.px; r.sy = s.py;
    place_positions(r, stream_key(seed, S_OBJ_POS, env, (uint32_t)s.episode), K, 2, [](int) {});
    s.gx = r.obj[1][0]; s.gy = r.obj[1][1];
    r.holding = r.held = start_holding ? 1 : 0;
    r.ox = start_holding ? s.px : r.obj[0][0];
    r.oy = start_holding ? s.py : r.obj[0][1];
    r.picks = 0;
    r.invalid = 0;
    float b;
    s.d_start = s.d_prev = rearr_potential(r, b);
}

// The task's free test: Nav2D-v0's, and outside the object's keep-out disc unless the object is held.  R, here and in rearr_pick and
// rearr_place: a Nav2DRearrState, or the geodesic step's RearrLane.
template <class R>
__device__ inline bool rearr_is_free(float x, float y, const R& r, int K) {
    return is_free(x, y, r.base, K) && (r.holding || !(dist(x, y, r.ox, r.oy) < OBJ_BLOCK));
}
// A PICK attempt with (c, sn) the heading's direction; returns whether it was the episode's first successful one.
template <class R>
__device__ inline bool rearr_pick(R& r, float c, float sn) {
    const auto& s = r.base;
    const float dx = r.ox - s.px, dy = r.oy - s.py;
    if (!r.holding && dist(s.px, s.py, r.ox, r.oy) < REARR_REACH && dx * c + dy * sn > 0.0f) {
        const bool first_pick = r.picks == 0;
        r.holding = r.held = 1;
        r.picks += 1;
        return first_pick;
    }
    r.invalid += 1;
    return false;
}
// A PLACE attempt with (c, sn) the heading's direction.
template <class R>
__device__ inline void rearr_place(R& r, float c, float sn, int K) {
    const auto& s = r.base;
    const float qx = s.px + REARR_ARM * c, qy = s.py + REARR_ARM * sn;
    if (r.holding && qx >= OBJ_LO && qx <= OBJ_HI && qy >= OBJ_LO && qy <= OBJ_HI && !in_grown_rect(qx, qy, s, K)) {
        r.ox = qx; r.oy = qy;
        r.holding = 0;
    } else {
        r.invalid += 1;
    }
}
// What follows the move of one step of this task, given the potential `phi` and its second term `b`: end_step_at's, with the
// potential in the distance's place, the pick bonus and this task's measures.  `stop` is the action's request to end the episode.
// Forced inline, as is rearr_end_step: left to itself the compiler makes it a call from both Euclidean kernels.
__device__ __forceinline__ void rearr_end_step_at(Nav2DRearrState& r, float phi, float b, bool stop, bool first_pick, float* __restrict__ reward,
                                                  uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed, uint32_t env, int n,
                                                  int N, int K, int nh, int max_steps, int start_holding) {
    Nav2DState& s = r.base;
    const bool success = stop && !r.holding && b < REARR_SUCCESS;
    reward[n] = ((-0.01f + (s.d_prev - phi)) + (first_pick ? 1.0f : 0.0f)) + (success ? 2.5f : 0.0f);
    s.d_prev = phi;
    s.steps += 1;
    const bool done = stop || (s.steps >= max_steps);
    not_done[n] = done ? 0 : 1;
    s.ended = done ? 1 : 0;
    if (done) {
        close_episode<false>(s, success ? 1.0f : 0.0f, (float)r.held, b, (float)s.collisions, sums, seed, env, n, N, K, nh);
        rearr_begin(r, seed, env, K, start_holding);
    }
}
// The end of a Euclidean step: a held object travels with the agent; then the potential of the straight lines, and the rest.
__device__ __forceinline__ void rearr_end_step(Nav2DRearrState& r, bool stop, bool first_pick, float* __restrict__ reward, uint8_t* __restrict__ not_done,
                                               float* __restrict__ sums, uint32_t seed, uint32_t env, int n, int N, int K, int nh, int max_steps,
                                               int start_holding) {
    if (r.holding) { r.ox = r.base.px; r.oy = r.base.py; }
    float b;
    const float phi = rearr_potential(r, b);
    rearr_end_step_at(r, phi, b, stop, first_pick, reward, not_done, sums, seed, env, n, N, K, nh, max_steps, start_holding);
}
// The three vector sensors: the object's start and the goal in the heading's frame, and the holding flag.
__device__ inline void rearr_write_sensors(const Nav2DRearrState& r, const float* __restrict__ dirs, float* __restrict__ obj_start,
                                           float* __restrict__ obj_goal, float* __restrict__ is_holding, int n) {
    const Nav2DState& s = r.base;
    const float c = dirs[2 * s.heading], sn = dirs[2 * s.heading + 1];
    if (obj_start) to_frame(r.obj[0][0] - s.px, r.obj[0][1] - s.py, c, sn, obj_start[2 * n + 0], obj_start[2 * n + 1]);
    if (obj_goal) to_frame(s.gx - s.px, s.gy - s.py, c, sn, obj_goal[2 * n + 0], obj_goal[2 * n + 1]);
    if (is_holding) is_holding[n] = (float)r.holding;
}

// One thread per env, as nav2d_step_kernel.  Then the three vector sensors.
__global__ void nav2d_rearr_step_kernel(Nav2DRearrState* __restrict__ states, const float* __restrict__ dirs,
                                        const int64_t* __restrict__ actions, const uint8_t* __restrict__ mask,
                                        float* __restrict__ obj_start, float* __restrict__ obj_goal, float* __restrict__ is_holding,
                                        float* __restrict__ reward, uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed,
                                        uint32_t env_offset, int N, int K, int nh, int max_steps, int start_holding, int advance) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (mask && !mask[n])) return;
    Nav2DRearrState& r = states[n];
    Nav2DState& s = r.base;
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        first_episode<false>(s, seed, env, K, nh);
        rearr_begin(r, seed, env, K, start_holding);
    } else {
        const int64_t a = actions[n];  // anything outside 0..5 moves nothing (the host-side entry points refuse it)
        const float c = dirs[2 * s.heading], sn = dirs[2 * s.heading + 1];
        bool first_pick = false;
        // discrete_move's statements, written out: through the call, with this task's free test, the kernel is no longer the
        // instructions it was (14 lines of mask arithmetic round the test), and this is one of the kernels held to that
        if (a == 1) {
            const float nx = s.px + FORWARD * c, ny = s.py + FORWARD * sn;
            if (rearr_is_free(nx, ny, r, K)) { s.px = nx; s.py = ny; s.path = s.path + FORWARD; }
            else s.collisions += 1;
        } else if (a == 2) {
            s.heading = (s.heading + 1) % nh;
        } else if (a == 3) {
            s.heading = (s.heading + nh - 1) % nh;
        } else if (a == 4) {
            first_pick = rearr_pick(r, c, sn);
        } else if (a == 5) {
            rearr_place(r, c, sn, K);
        }
        rearr_end_step(r, a == 0, first_pick, reward, not_done, sums, seed, env, n, N, K, nh, max_steps, start_holding);
    }
    rearr_write_sensors(r, dirs, obj_start, obj_goal, is_holding, n);
}

// Nav2DRearrVel-v0 (Nav2DRearrVelVectorEnv; specification: tests/nav2d_rearr_vel_reference.py): Nav2DRearr-v0's record, world, places,
// reward, measures and sensors under Nav2DVel-v0's velocity control plus a grip component.  The action (a_lin, a_ang, a_grip) is one
// 12-byte row of an (N, 3) float32 tensor, read as three scalars: a row is 4-byte aligned and no more.  The motion is vel_decode /
// vel_move with this task's free test; then, on every step, the grip with the new position and heading: c_grip > 0 with empty hands
// is a PICK attempt, c_grip < 0 while holding a PLACE attempt, every other combination nothing; then Nav2DRearr-v0's end of the step
// with the velocity stop in STOP's place.  A step of this task tests up to three positions, so it tests them on FreeBoxes.
__global__ void __launch_bounds__(64)
nav2d_rearr_vel_step_kernel(Nav2DRearrState* __restrict__ states, const float* __restrict__ dirs, const float* __restrict__ actions,
                            const uint8_t* __restrict__ mask, float* __restrict__ obj_start, float* __restrict__ obj_goal,
                            float* __restrict__ is_holding, float* __restrict__ reward, uint8_t* __restrict__ not_done,
                            float* __restrict__ sums, uint32_t seed, uint32_t env_offset, int N, int K, int nh, int max_steps,
                            int start_holding, int max_turn, int stop_turn, float min_lin, int sliding, int advance) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (mask && !mask[n])) return;
    Nav2DRearrState& r = states[n];
    Nav2DState& s = r.base;
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        first_episode<false>(s, seed, env, K, nh);
        rearr_begin(r, seed, env, K, start_holding);
    } else {
        const float a_lin = actions[3 * (size_t)n], a_ang = actions[3 * (size_t)n + 1], c_grip = vel_clamp(actions[3 * (size_t)n + 2]);
        float l;
        int dh;
        const bool stop = vel_decode(a_lin, a_ang, max_turn, stop_turn, min_lin, l, dh);
        if (!stop) {
            FreeBoxes boxes;
            load_free_boxes(boxes, s, K);
            const bool holding = r.holding;
            const float ox = r.ox, oy = r.oy;  // neither moves during the move: a held object follows at the end of the step
            vel_move(s, dirs, l, dh, nh, sliding, [&](float x, float y) {  // rearr_is_free, on the registers
                return is_free_boxes(x, y, boxes, K) && (holding || !(dist(x, y, ox, oy) < OBJ_BLOCK));
            });
        }
        const float c = dirs[2 * s.heading], sn = dirs[2 * s.heading + 1];
        bool first_pick = false;
        if (c_grip > 0.0f && !r.holding) first_pick = rearr_pick(r, c, sn);
        else if (c_grip < 0.0f && r.holding) rearr_place(r, c, sn, K);
        rearr_end_step(r, stop, first_pick, reward, not_done, sums, seed, env, n, N, K, nh, max_steps, start_holding);
    }
    rearr_write_sensors(r, dirs, obj_start, obj_goal, is_holding, n);
}

// ---- geodesic distance of Nav2DObj-v0 (distance = "geodesic"; specification: tests/nav2d_obj_geo_reference.py) ---------------------
// The distance to the nearest instance of the target category along the shortest path.  Obstacles of the graph: the K rectangles
// grown by the agent radius and, for each object, the bounding square of its keep-out disc, up to 16 boxes; 64 nodes, 4k + j corner j
// of rectangle box k, 32 + 4m + j corner j of object m's square; targets, the centres of the objects of the target category, each
// seen through its own square.  The field of one env's running episode (HAB_NAV2D_OBJ_GEO_BYTES) is GeoField's layout over 64 nodes.
constexpr int OBJ_GEO_NODES = GEO_NODES + 4 * MAX_M, OBJ_GEO_BOXES = MAX_K + MAX_M;
static_assert(OBJ_GEO_NODES == 64, "one node per lane of a wavefront");
using ObjGeoField = GeoFieldOf<OBJ_GEO_NODES>;
static_assert(sizeof(ObjGeoField) == HAB_NAV2D_OBJ_GEO_BYTES, "ObjGeoField layout");
static_assert(offsetof(ObjGeoField, reachable) == 4 * HAB_NAV2D_OBJ_GEO_W_REACHABLE &&
              offsetof(ObjGeoField, sweeps) == 4 * HAB_NAV2D_OBJ_GEO_W_SWEEPS &&
              offsetof(ObjGeoField, lost_steps) == 4 * HAB_NAV2D_OBJ_GEO_W_LOST_STEPS, "ObjGeoField layout");

// Node i of the graph; false where it does not exist (k >= K, m >= M).
__device__ inline bool obj_geo_node(const Nav2DObjState& o, int i, int K, int M, float& x, float& y) {
    x = 0.0f; y = 0.0f;
    if (i < GEO_NODES) {
        if (i >= 4 * K) return false;
        geo_corner(o.base, i >> 2, i & 3, x, y);
        return true;
    }
    const int m = (i - GEO_NODES) >> 2, j = i & 3;
    if (m >= M) return false;
    x = (j & 1) ? o.obj[m][0] + OBJ_BLOCK : o.obj[m][0] - OBJ_BLOCK;
    y = (j & 2) ? o.obj[m][1] + OBJ_BLOCK : o.obj[m][1] - OBJ_BLOCK;
    return true;
}
// Object m's visibility box: its square shrunk by GEO_E.
__device__ inline GeoBox obj_geo_box(const Nav2DObjState& o, int m) {
    return geo_box(o.obj[m][0] - OBJ_BLOCK, o.obj[m][1] - OBJ_BLOCK, o.obj[m][0] + OBJ_BLOCK, o.obj[m][1] + OBJ_BLOCK);
}
// The K + M visibility boxes into the wave's LDS array, rectangles first; the caller puts the barrier after it.
__device__ inline void obj_geo_fill_boxes(GeoBox* boxes, const Nav2DObjState& o, int K, int M, int lane) {
    if (lane < K) boxes[lane] = geo_box(o.base, lane);
    else if (lane >= MAX_K && lane - MAX_K < M) boxes[K + (lane - MAX_K)] = obj_geo_box(o, lane - MAX_K);
}
// Whether a-b misses the B boxes, box `skip` left out.
__device__ inline bool geo_visible_but(const GeoBox* boxes, int B, int skip, float ax, float ay, float bx, float by) {
    for (int b = 0; b < B; ++b)
        if (b != skip && geo_blocked(boxes[b], ax, ay, bx, by)) return false;
    return true;
}
// geo(p) by one wavefront: lane i takes node i = (x, y) with field value Di (+inf: no candidate), lane t < M also the centre of
// object t where it is a target, seen with its own box left out; then the minimum over the wave, which is exact and so the
// restatement's serial one.
__device__ inline float obj_geo_query(const Nav2DObjState& o, const GeoBox* boxes, int K, int M, float px, float py, float x, float y,
                                      float Di, int lane) {
    float v = INFINITY;
    if (Di < INFINITY && geo_visible(boxes, K + M, px, py, x, y)) v = dist(px, py, x, y) + Di;
    if (lane < M && o.cat[lane] == o.target) {
        const float cx = o.obj[lane][0], cy = o.obj[lane][1];
        if (geo_visible_but(boxes, K + M, K + lane, px, py, cx, cy)) v = fminf(v, dist(px, py, cx, cy));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}

// The field of one env per 64-thread workgroup (one wavefront), selected like nav2d_geo_build_kernel's.  Lane i owns node i.  The
// weights are one symmetric 64 x 64 matrix in LDS (16 KiB), each of the 2016 node pairs tested once -- geo_blocked and dist are
// bitwise symmetric in their two points -- and written to both places: a lane that computed its own row of 63 would run twice the
// visibility tests, and they are what the kernel's time is.  The pairs go round the lanes in 32 rounds: rows a and 62 - a hold 64
// pairs together, row 31 alone 32.  A sweep is 64 add / min per lane on its column of the matrix (row j of the array is one dword
// per lane: no bank conflict) and D (a broadcast read), the two copies of D as in geo_field_towards, then a wave vote.
__global__ void __launch_bounds__(64)
nav2d_obj_geo_build_kernel(char* __restrict__ states, size_t state_stride, ObjGeoField* __restrict__ geo, const uint8_t* __restrict__ mask,
                           int only_ended, int K, int M) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    Nav2DObjState& o = *reinterpret_cast<Nav2DObjState*>(states + (size_t)n * state_stride);
    Nav2DState& s = o.base;
    if (only_ended && !s.ended) return;
    __shared__ float node_x[OBJ_GEO_NODES], node_y[OBJ_GEO_NODES];
    __shared__ int node_ok[OBJ_GEO_NODES];
    __shared__ GeoBox boxes[OBJ_GEO_BOXES];
    __shared__ float W[OBJ_GEO_NODES * OBJ_GEO_NODES];
    __shared__ float D[2][OBJ_GEO_NODES];
    float x, y;
    const bool ok = obj_geo_node(o, lane, K, M, x, y) && is_free_obj(x, y, o, K, M);
    node_x[lane] = x; node_y[lane] = y; node_ok[lane] = ok ? 1 : 0;
    W[lane * OBJ_GEO_NODES + lane] = INFINITY;
    obj_geo_fill_boxes(boxes, o, K, M, lane);
    __syncthreads();
    const int B = K + M;
    for (int p = lane; p < OBJ_GEO_NODES * (OBJ_GEO_NODES - 1) / 2; p += 64) {
        const int a = p >> 6, c = p & 63;
        const int i = c < 63 - a ? a : 62 - a;
        const int j = c < 63 - a ? a + 1 + c : i + 1 + (c - (63 - a));
        float w = INFINITY;
        if (node_ok[i] && node_ok[j] && geo_visible(boxes, B, node_x[i], node_y[i], node_x[j], node_y[j]))
            w = dist(node_x[i], node_y[i], node_x[j], node_y[j]);
        W[i * OBJ_GEO_NODES + j] = w;
        W[j * OBJ_GEO_NODES + i] = w;
    }
    // the last hop: the nearest of the target centres the node sees, each through its own square
    float d = INFINITY;
    if (ok) {
        for (int t = 0; t < M; ++t) {
            if (o.cat[t] != o.target) continue;
            const float cx = o.obj[t][0], cy = o.obj[t][1];
            if (geo_visible_but(boxes, B, K + t, x, y, cx, cy)) d = fminf(d, dist(x, y, cx, cy));
        }
    }
    D[0][lane] = d;
    __syncthreads();
    int cur = 0, sweeps = 0;
    while (sweeps < 4 * B) {  // uniform over the wave: K and M are arguments, the exit a vote
        sweeps += 1;
        float m = INFINITY;
        for (int j = 0; j < OBJ_GEO_NODES; ++j) m = fminf(m, W[j * OBJ_GEO_NODES + lane] + D[cur][j]);
        const float before = D[cur][lane];
        const float after = fminf(before, m);
        D[cur ^ 1][lane] = after;
        const bool changed = __ballot(after != before) != 0;
        __syncthreads();
        cur ^= 1;
        if (!changed) break;
    }
    const float Di = D[cur][lane];
    geo[n].D[lane] = Di;
    const float v = obj_geo_query(o, boxes, K, M, s.px, s.py, x, y, Di, lane);  // g0 = geo(current position)
    __syncthreads();  // every lane has read the state before lane 0 writes to it
    if (lane == 0) {
        const bool reachable = v < INFINITY;
        geo[n].reachable = reachable ? 1 : 0;
        geo[n].sweeps = sweeps;
        geo[n].lost_steps = 0;
        for (int z = 0; z < 5; ++z) geo[n].zero[z] = 0;
        if (reachable) s.d_start = s.d_prev = v;
    }
}

// The geodesic form of the object step: one wavefront (a 64-thread workgroup) per env.  Every lane derives the move on its own
// MoveLane from the same loads, so the outcome is uniform and lane 0 alone writes it back; the query of the new position takes one
// node per lane plus the targets and a wave minimum; lane 0 then does what nav2d_obj_step_kernel does after its move, with that
// distance.  The field of an episode that begins here is built by the launch of nav2d_obj_geo_build_kernel that follows (only_ended).
__global__ void __launch_bounds__(64)
nav2d_obj_geo_step_kernel(Nav2DObjState* __restrict__ states, ObjGeoField* __restrict__ geo, const float* __restrict__ dirs,
                          const float* __restrict__ ctab, const int64_t* __restrict__ actions, const uint8_t* __restrict__ mask,
                          int64_t* __restrict__ objectgoal, float* __restrict__ gps, float* __restrict__ compass,
                          float* __restrict__ reward, uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed,
                          uint32_t env_offset, int N, int K, int nh, int max_steps, int M, int C, int advance) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    Nav2DObjState& o = states[n];
    Nav2DState& s = o.base;
    ObjGeoField& g = geo[n];
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        if (lane == 0) {
            first_episode<false>(s, seed, env, K, nh);
            place_objects(o, seed, env, K, M, C);
        }
    } else {
        __shared__ GeoBox boxes[OBJ_GEO_BOXES];
        const int64_t a = actions[n];
        MoveLane m = load_move(s);  // this lane's copy
        discrete_move(m, a, dirs, nh, [&](float x, float y) { return is_free_obj(x, y, o, K, M); });
        const bool reachable = g.reachable != 0;  // of the env, so uniform over the workgroup
        float d = INFINITY;
        if (reachable) {
            obj_geo_fill_boxes(boxes, o, K, M, lane);
            __syncthreads();
            float x, y;
            const float Di = obj_geo_node(o, lane, K, M, x, y) ? g.D[lane] : INFINITY;
            d = obj_geo_query(o, boxes, K, M, m.px, m.py, x, y, Di, lane);
        }
        __syncthreads();  // every lane has read the state and the field before lane 0 writes to them
        if (lane == 0) {
            store_move(s, m);
            const float straight = nearest_target(o, M);  // (gx, gy) stay the Euclidean-nearest centre
            if (!reachable) d = straight;
            else if (!(d < INFINITY)) { d = s.d_prev; g.lost_steps += 1; }
            end_step_at<false>(s, d, a == 0, OBJ_SUCCESS, reward, not_done, sums, seed, env, n, N, K, nh, max_steps);
            if (s.ended) place_objects(o, seed, env, K, M, C);
        }
    }
    if (lane == 0) obj_write_sensors(o, dirs, ctab, objectgoal, gps, compass, n, nh);
}

// ---- geodesic distances of Nav2DRearr-v0 and Nav2DRearrVel-v0 (distance = "geodesic"; specification: --------------------------------
// tests/nav2d_rearr_geo_reference.py) ------------------------------------------------------------------------------------------------
// The two terms of the potential along shortest paths over Nav2D-v0's graph (the object is no obstacle of it): a = geo_o(p), 0 while
// the object is held, and b = geo_g(o), evaluated when the object comes to rest and kept while it rests, geo_g(p) while it is held.
// The record of one env's running episode (HAB_NAV2D_REARR_GEO_BYTES): the field DG towards the goal, the field DO towards the place
// where the object rests (+inf while it has not rested in the episode), the two terms after the last step and the counters.
struct RearrGeoField {
    float DG[GEO_NODES], DO[GEO_NODES];
    float a, b;
    int32_t reachable, sweeps_goal, sweeps_obj, lost_steps, rebuilds, zero;
};
static_assert(sizeof(RearrGeoField) == HAB_NAV2D_REARR_GEO_BYTES, "RearrGeoField layout");
static_assert(offsetof(RearrGeoField, DG) == 4 * HAB_NAV2D_REARR_GEO_W_DG && offsetof(RearrGeoField, DO) == 4 * HAB_NAV2D_REARR_GEO_W_DO,
              "RearrGeoField layout");
static_assert(offsetof(RearrGeoField, a) == 4 * HAB_NAV2D_REARR_GEO_W_A && offsetof(RearrGeoField, b) == 4 * HAB_NAV2D_REARR_GEO_W_B,
              "RearrGeoField layout");
static_assert(offsetof(RearrGeoField, reachable) == 4 * HAB_NAV2D_REARR_GEO_W_REACHABLE &&
              offsetof(RearrGeoField, sweeps_goal) == 4 * HAB_NAV2D_REARR_GEO_W_SWEEPS_GOAL &&
              offsetof(RearrGeoField, sweeps_obj) == 4 * HAB_NAV2D_REARR_GEO_W_SWEEPS_OBJ, "RearrGeoField layout");
static_assert(offsetof(RearrGeoField, lost_steps) == 4 * HAB_NAV2D_REARR_GEO_W_LOST_STEPS &&
              offsetof(RearrGeoField, rebuilds) == 4 * HAB_NAV2D_REARR_GEO_W_REBUILDS, "RearrGeoField layout");

// What the beginning of an episode needs, one env per 64-thread workgroup (one wavefront), selected like nav2d_geo_build_kernel's.
// `state` is a record that rearr_begin has just filled: the object is at its start, or at the agent's position under start_holding.
// Nodes, boxes and weights are computed once and serve both fields.  DG, then b0 = geo_g(o); without start_holding DO towards o and
// a0 = geo_o(p), with it DO = +inf, no sweeps and a0 = 0.  Both terms finite: reachable, and d_start = d_prev = a0 + b0.
__global__ void __launch_bounds__(64)
nav2d_rearr_geo_build_kernel(char* __restrict__ states, size_t state_stride, RearrGeoField* __restrict__ geo, const uint8_t* __restrict__ mask,
                             int only_ended, int K, int start_holding) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    Nav2DRearrState& r = *reinterpret_cast<Nav2DRearrState*>(states + (size_t)n * state_stride);
    Nav2DState& s = r.base;
    if (only_ended && !s.ended) return;
    __shared__ GeoGraph G;
    geo_graph_nodes(G, s, K, lane);
    __syncthreads();
    geo_graph_weights(G, K, lane);
    const float px = s.px, py = s.py, gx = s.gx, gy = s.gy, ox = r.ox, oy = r.oy;
    __syncthreads();
    float Dg, Do = INFINITY;
    const int sweeps_goal = geo_field_towards(G, K, gx, gy, lane, Dg);
    const float b0 = geo_query_wave(G, K, ox, oy, gx, gy, Dg, lane);
    int sweeps_obj = 0;
    float a0 = 0.0f;
    if (!start_holding) {
        sweeps_obj = geo_field_towards(G, K, ox, oy, lane, Do);
        a0 = geo_query_wave(G, K, px, py, ox, oy, Do, lane);
    }
    RearrGeoField& g = geo[n];
    if (lane < GEO_NODES) { g.DG[lane] = Dg; g.DO[lane] = Do; }
    __syncthreads();  // every lane has read the state before lane 0 writes to it
    if (lane == 0) {
        const bool reachable = (a0 < INFINITY) && (b0 < INFINITY);
        g.a = a0; g.b = b0;
        g.reachable = reachable ? 1 : 0;
        g.sweeps_goal = sweeps_goal;
        g.sweeps_obj = sweeps_obj;
        g.lost_steps = 0;
        g.rebuilds = 0;
        g.zero = 0;
        if (reachable) s.d_start = s.d_prev = a0 + b0;
    }
}

// rearr_end_step_at for the geodesic step, which has its potential and its second term already.  Not forced inline: the compiler makes
// it one function that both forms of the step kernel call, and forced into them it grows each by half.
__device__ inline void rearr_geo_end_step(Nav2DRearrState& r, float phi, float b, bool stop, bool first_pick, float* __restrict__ reward,
                                          uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed, uint32_t env, int n, int N,
                                          int K, int nh, int max_steps, int start_holding) {
    rearr_end_step_at(r, phi, b, stop, first_pick, reward, not_done, sums, seed, env, n, N, K, nh, max_steps, start_holding);
}

// What a step changes of a record before its end, as a lane's own copy in registers, with the rectangles, which it does not change,
// behind a pointer to the record: the members the motion, PICK and PLACE helpers read and write.  A copy of the whole record would be
// indexed by k and live in scratch memory.
struct RearrLane {
    struct Base : MoveLane {
        const float (*rect)[4];
    } base;
    float ox, oy;
    int32_t holding, held, picks, invalid;
};

// The geodesic form of both rearrangement steps: one wavefront (a 64-thread workgroup) per env, as nav2d_obj_geo_step_kernel.  Every
// lane takes its own copy of the record's changing words and derives the move, the PICK or the PLACE on it through the helpers of the
// Euclidean kernels, from the same loads, so the outcome is uniform over the wave; lane 0 alone writes it back.  In a reachable episode the
// nodes and boxes go to LDS and the terms are queries of one node per lane; a successful PLACE first builds DO towards the new
// resting place, the weights included.  Lane 0 then applies the lost-step rule and does the end of the step.  The fields of an
// episode that begins here are built by the launch of nav2d_rearr_geo_build_kernel that follows (only_ended).
// VEL: `actions` are Nav2DRearrVel-v0's (N, 3) float rows and the four motion parameters are used; else int64 actions.
template <bool VEL>
__global__ void __launch_bounds__(64)
nav2d_rearr_geo_step_kernel(Nav2DRearrState* __restrict__ states, RearrGeoField* __restrict__ geo, const float* __restrict__ dirs,
                            const void* __restrict__ actions, const uint8_t* __restrict__ mask, float* __restrict__ obj_start,
                            float* __restrict__ obj_goal, float* __restrict__ is_holding, float* __restrict__ reward,
                            uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed, uint32_t env_offset, int N, int K,
                            int nh, int max_steps, int start_holding, int max_turn, int stop_turn, float min_lin, int sliding, int advance) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    Nav2DRearrState& rec = states[n];
    RearrGeoField& g = geo[n];
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        if (lane == 0) {
            first_episode<false>(rec.base, seed, env, K, nh);
            rearr_begin(rec, seed, env, K, start_holding);
        }
    } else {
        __shared__ GeoGraph G;
        RearrLane r{{load_move(rec.base), rec.base.rect}, rec.ox, rec.oy, rec.holding, rec.held, rec.picks, rec.invalid};  // this lane's copy
        RearrLane::Base& s = r.base;
        const float gx = rec.base.gx, gy = rec.base.gy;
        const bool was_holding = r.holding != 0;
        bool stop, first_pick = false;
        if constexpr (VEL) {
            const float* act = static_cast<const float*>(actions) + 3 * (size_t)n;
            const float a_lin = act[0], a_ang = act[1], c_grip = vel_clamp(act[2]);
            float l;
            int dh;
            stop = vel_decode(a_lin, a_ang, max_turn, stop_turn, min_lin, l, dh);
            if (!stop) vel_move(s, dirs, l, dh, nh, sliding, [&](float x, float y) { return rearr_is_free(x, y, r, K); });
            const float c = dirs[2 * s.heading], sn = dirs[2 * s.heading + 1];
            if (c_grip > 0.0f && !r.holding) first_pick = rearr_pick(r, c, sn);
            else if (c_grip < 0.0f && r.holding) rearr_place(r, c, sn, K);
        } else {
            const int64_t a = static_cast<const int64_t*>(actions)[n];
            const float c = dirs[2 * s.heading], sn = dirs[2 * s.heading + 1];
            discrete_move(s, a, dirs, nh, [&](float x, float y) { return rearr_is_free(x, y, r, K); });
            if (a == 4) first_pick = rearr_pick(r, c, sn);
            else if (a == 5) rearr_place(r, c, sn, K);
            stop = a == 0;
        }
        if (r.holding) { r.ox = s.px; r.oy = s.py; }
        const bool placed = was_holding && !r.holding;  // the object came to rest in this step
        const bool reachable = g.reachable != 0;        // of the env, so uniform over the workgroup
        float ta = g.a, tb = g.b;                       // the terms after the previous step
        float na = 0.0f, nb = tb, Do = INFINITY;
        int sweeps_obj = 0;
        if (reachable) {
            geo_graph_nodes(G, rec.base, K, lane);
            __syncthreads();
            const float Dg = lane < GEO_NODES ? g.DG[lane] : INFINITY;
            if (placed) {
                geo_graph_weights(G, K, lane);
                __syncthreads();
                sweeps_obj = geo_field_towards(G, K, r.ox, r.oy, lane, Do);
                nb = geo_query_wave(G, K, r.ox, r.oy, gx, gy, Dg, lane);
                na = geo_query_wave(G, K, s.px, s.py, r.ox, r.oy, Do, lane);
            } else if (r.holding) {
                nb = geo_query_wave(G, K, s.px, s.py, gx, gy, Dg, lane);
            } else {
                Do = lane < GEO_NODES ? g.DO[lane] : INFINITY;
                na = geo_query_wave(G, K, s.px, s.py, r.ox, r.oy, Do, lane);
            }
        }
        __syncthreads();  // every lane has read the record and the field before lane 0 writes to them
        if (reachable && placed && lane < GEO_NODES) g.DO[lane] = Do;
        if (lane == 0) {
            store_move(rec.base, s);
            rec.ox = r.ox; rec.oy = r.oy;
            rec.holding = r.holding; rec.held = r.held; rec.picks = r.picks; rec.invalid = r.invalid;
            float phi, b;
            if (reachable) {
                const bool lost = !(na < INFINITY) || !(nb < INFINITY);
                if (na < INFINITY) ta = na;
                if (nb < INFINITY) tb = nb;
                g.a = ta; g.b = tb;
                if (lost) g.lost_steps += 1;
                if (placed) { g.sweeps_obj = sweeps_obj; g.rebuilds += 1; }
                phi = ta + tb;
                b = tb;
            } else {
                phi = rearr_potential(rec, b);  // of the record as just written
            }
            rearr_geo_end_step(rec, phi, b, stop, first_pick, reward, not_done, sums, seed, env, n, N, K, nh, max_steps, start_holding);
        }
    }
    if (lane == 0) rearr_write_sensors(rec, dirs, obj_start, obj_goal, is_holding, n);
}

// ---- the pick-and-place oracle of Nav2DRearr-v0 in geodesic mode (specification: tests/nav2d_rearr_oracle_reference.py) -------------
// One env per 64-thread workgroup (one wavefront), selected by `mask` (NULL: all); lane = candidate heading, the lanes stride over
// the nh headings by 64, as in forward_search.  State and field are read only, through pointers that are uniform over the wave,
// and so are `holding` and "in reach": an env runs one of three paths.
//   * Not holding, in reach: the dot test of rearr_pick per heading; the fewest turns win.
//   * Not holding, out of reach: forward_search towards o over DO below the term a, with the task's free test.
//   * Holding: the place search -- q of rearr_place per heading, eligible where the PLACE would be accepted and w = geo_g(q) < 0.5;
//     the fewest turns win -- and, where no heading is eligible, the forward search towards g over DG below the term b.
// Both forward searches are one call with a uniform field pointer, target and bound, so a lane runs at most two straight-line
// queries per pass of the lanes: one of the place search, one of the forward search.  The two turn-only searches have the turn key in the high word and w's bits (0 for the dot test) in the low
// word, which the minimum carries along for next_d.  One wave-wide minimum per search; lane 0 writes action, next_d and status.
__global__ void __launch_bounds__(64)
nav2d_rearr_oracle_kernel(const char* __restrict__ states, size_t state_stride, const RearrGeoField* __restrict__ geo,
                          const float* __restrict__ dirs, const uint8_t* __restrict__ mask, int64_t* __restrict__ actions,
                          float* __restrict__ next_d, int32_t* __restrict__ status, int K, int nh) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    const Nav2DRearrState& r = *reinterpret_cast<const Nav2DRearrState*>(states + (size_t)n * state_stride);
    const Nav2DState& s = r.base;
    const RearrGeoField& g = geo[n];
    const float px = s.px, py = s.py, ta = g.a, tb = g.b;
    const int heading = s.heading;
    const bool holding = r.holding != 0;
    int st = HAB_NAV2D_ORACLE_STUCK, delta = 0;
    float nd = INFINITY;
    const float* D = nullptr;  // the forward search's field: set where the env's path comes to it
    float tx = 0.0f, ty = 0.0f, bound = 0.0f;
    if (!g.reachable) {
        st = HAB_NAV2D_ORACLE_UNREACHABLE;
    } else if (!holding && tb < REARR_SUCCESS) {
        st = HAB_NAV2D_ORACLE_ARRIVED;
        nd = tb;
    } else if (!holding && dist(px, py, r.ox, r.oy) < REARR_REACH) {
        const float dx = r.ox - px, dy = r.oy - py;
        unsigned long long key = NO_KEY;
        for (int h0 = 0; h0 < nh; h0 += 64) {  // uniform over the wave
            const int h = h0 + lane;
            if (h >= nh) continue;
            if (!(dx * dirs[2 * h] + dy * dirs[2 * h + 1] > 0.0f)) continue;
            const unsigned long long k = (unsigned long long)turn_key(h, heading, nh) << 32;
            key = k < key ? k : key;
        }
        key = wave_min_key(key);
        if (key != NO_KEY) {
            delta = turn_key_delta((uint32_t)(key >> 32));
            st = delta == 0 ? HAB_NAV2D_ORACLE_PICK : HAB_NAV2D_ORACLE_GO;
            nd = delta == 0 ? 0.0f : ta;
        }
    } else if (!holding) {
        D = g.DO; tx = r.ox; ty = r.oy; bound = ta;
    } else {
        unsigned long long key = NO_KEY;
        for (int h0 = 0; h0 < nh; h0 += 64) {
            const int h = h0 + lane;
            if (h >= nh) continue;
            const float qx = px + REARR_ARM * dirs[2 * h], qy = py + REARR_ARM * dirs[2 * h + 1];
            if (!(qx >= OBJ_LO && qx <= OBJ_HI && qy >= OBJ_LO && qy <= OBJ_HI) || in_grown_rect(qx, qy, s, K)) continue;
            const float w = geo_query(s, g.DG, K, qx, qy, s.gx, s.gy);
            if (!(w < INFINITY && w < REARR_SUCCESS)) continue;
            const unsigned long long k = ((unsigned long long)turn_key(h, heading, nh) << 32) | __float_as_uint(w);
            key = k < key ? k : key;
        }
        key = wave_min_key(key);
        if (key != NO_KEY) {
            delta = turn_key_delta((uint32_t)(key >> 32));
            st = delta == 0 ? HAB_NAV2D_ORACLE_PLACE : HAB_NAV2D_ORACLE_GO;
            nd = delta == 0 ? __uint_as_float((uint32_t)key) : tb;
        } else {
            D = g.DG; tx = s.gx; ty = s.gy; bound = tb;
        }
    }
    if (D) {
        const unsigned long long key =
            forward_search(s, D, dirs, K, nh, tx, ty, bound, lane, [&](float x, float y) { return rearr_is_free(x, y, r, K); });
        if (key != NO_KEY) {
            st = HAB_NAV2D_ORACLE_GO;
            delta = turn_key_delta((uint32_t)key);
            nd = delta == 0 ? __uint_as_float((uint32_t)(key >> 32)) : bound;  // a turn leaves the leg's term as it is
        }
    }
    if (lane == 0) {
        actions[n] = st == HAB_NAV2D_ORACLE_GO ? FollowDiscrete{}(true, delta) : st == HAB_NAV2D_ORACLE_PICK ? 4 : st == HAB_NAV2D_ORACLE_PLACE ? 5 : 0;
        if (next_d) next_d[n] = nd;
        if (status) status[n] = st;
    }
}

// ---- Nav2DSocial-v0 (Nav2DSocialVectorEnv; specification: tests/nav2d_social_reference.py) ------------------------------------------
// A person walks about Nav2D-v0's world, from waypoint to waypoint along the shortest paths of Nav2D-v0's graph, and the agent has to
// find and then to follow them under Nav2DVel-v0's velocity control.  The graph is planned with here: the person's hop is the
// arg-min of the wave query, and the field towards a new waypoint is built inside the step that reaches the old one.
constexpr uint32_t S_WAYPOINT = 24u;
constexpr float SOCIAL_NEAR = 1.0f, SOCIAL_FAR = 2.0f;

// One env of Nav2DSocial-v0: a Nav2D-v0 record ((gx, gy) zero, d_prev = d(p, h) after the last step, d_start = the episode's first),
// then the agent's start, the person's position h (named as place_positions reads it), the waypoint and its index in the episode,
// the found flag, the episode's counters and the field DW towards the waypoint.
struct Nav2DSocialState {
    Nav2DState base;
    float sx, sy;
    float obj[1][2];            // the person (x, y)
    float wx, wy;
    int32_t wp_index, found, following_steps, first_encounter;
    int32_t arrivals, person_waits, person_lost, sweeps, rebuilds, zero;
    float DW[GEO_NODES];
};
static_assert(sizeof(Nav2DSocialState) == HAB_NAV2D_SOCIAL_STATE_BYTES && offsetof(Nav2DSocialState, base) == 0, "Nav2DSocialState layout");
static_assert(offsetof(Nav2DSocialState, sx) == 4 * HAB_NAV2D_SOCIAL_W_START && offsetof(Nav2DSocialState, sy) == 4 * HAB_NAV2D_SOCIAL_W_START + 4,
              "Nav2DSocialState layout");
static_assert(offsetof(Nav2DSocialState, obj) == 4 * HAB_NAV2D_SOCIAL_W_PERSON && offsetof(Nav2DSocialState, wx) == 4 * HAB_NAV2D_SOCIAL_W_WAYPOINT &&
              offsetof(Nav2DSocialState, wy) == 4 * HAB_NAV2D_SOCIAL_W_WAYPOINT + 4, "Nav2DSocialState layout");
static_assert(offsetof(Nav2DSocialState, wp_index) == 4 * HAB_NAV2D_SOCIAL_W_WAYPOINT_INDEX && offsetof(Nav2DSocialState, found) == 4 * HAB_NAV2D_SOCIAL_W_FOUND,
              "Nav2DSocialState layout");
static_assert(offsetof(Nav2DSocialState, following_steps) == 4 * HAB_NAV2D_SOCIAL_W_FOLLOWING_STEPS &&
              offsetof(Nav2DSocialState, first_encounter) == 4 * HAB_NAV2D_SOCIAL_W_FIRST_ENCOUNTER, "Nav2DSocialState layout");
static_assert(offsetof(Nav2DSocialState, arrivals) == 4 * HAB_NAV2D_SOCIAL_W_ARRIVALS && offsetof(Nav2DSocialState, person_waits) == 4 * HAB_NAV2D_SOCIAL_W_PERSON_WAITS &&
              offsetof(Nav2DSocialState, person_lost) == 4 * HAB_NAV2D_SOCIAL_W_PERSON_LOST, "Nav2DSocialState layout");
static_assert(offsetof(Nav2DSocialState, sweeps) == 4 * HAB_NAV2D_SOCIAL_W_SWEEPS && offsetof(Nav2DSocialState, rebuilds) == 4 * HAB_NAV2D_SOCIAL_W_REBUILDS &&
              offsetof(Nav2DSocialState, DW) == 4 * HAB_NAV2D_SOCIAL_W_DW, "Nav2DSocialState layout");

// Waypoint j of the episode whose key of stream 24 is `kw`, for a person at (hx, hy): the first of its 16 candidates, else the first
// ring slot, inside [0.5, 7.5]^2, not strictly inside a rectangle grown by 0.3 m and at least 1 m from the person.  An open disc of
// radius 1 holds at most three ring slots, so one always fits.  S: a record with the rectangles.
template <class S>
__device__ inline void social_waypoint(const S& s, uint32_t kw, int K, int j, float hx, float hy, float& wx, float& wy) {
    auto fits = [&](float x, float y) {
        return x >= OBJ_LO && x <= OBJ_HI && y >= OBJ_LO && y <= OBJ_HI && !in_grown_rect(x, y, s, K) && dist(hx, hy, x, y) >= OBJ_APART;
    };
    for (int i = 0; i < CANDIDATES; ++i) {
        const uint32_t w = 2u * ((uint32_t)CANDIDATES * (uint32_t)j + (uint32_t)i);
        wx = LO + 7.8f * u01(mix32(kw ^ w)); wy = LO + 7.8f * u01(mix32(kw ^ (w + 1u)));
        if (fits(wx, wy)) return;
    }
    for (int q = 0; q < RING_SLOTS; ++q) {
        ring_slot(q, wx, wy);
        if (fits(wx, wy)) return;
    }
}
// What Nav2DSocial-v0 adds to a world that `begin_episode<false>` has just generated: the person where Nav2DObj-v0 puts object 0 of
// that world with one object, waypoint 0, the counters and the first distance.  The field is built by nav2d_social_build_kernel.
__device__ inline void social_begin(Nav2DSocialState& r, uint32_t seed, uint32_t env, int K) {
    Nav2DState& s = r.base;
    const uint32_t ep = (uint32_t)s.episode;
    r.sx = s.px; r.sy = s.py;
    place_positions(r, stream_key(seed, S_OBJ_POS, env, ep), K, 1, [](int) {});
    s.gx = 0.0f; s.gy = 0.0f;
    r.wp_index = 0;
    social_waypoint(s, stream_key(seed, S_WAYPOINT, env, ep), K, 0, r.obj[0][0], r.obj[0][1], r.wx, r.wy);
    r.found = r.following_steps = r.first_encounter = 0;
    r.arrivals = r.person_waits = r.person_lost = r.sweeps = r.rebuilds = r.zero = 0;
    s.d_start = s.d_prev = dist(s.px, s.py, r.obj[0][0], r.obj[0][1]);
}
// (dot, cross) of h - p in the heading's frame, and whether the agent sees the person: inside the camera's 90 degree field of view
// and visible over the graph's boxes.  By one thread, the boxes through the record.
__device__ inline bool social_sees(const Nav2DSocialState& r, const float* __restrict__ dirs, int K, float& dot, float& cross) {
    const Nav2DState& s = r.base;
    const float c = dirs[2 * s.heading], sn = dirs[2 * s.heading + 1];
    const float hx = r.obj[0][0], hy = r.obj[0][1];
    to_frame(hx - s.px, hy - s.py, c, sn, dot, cross);
    if (!(dot > 0.0f && fabsf(cross) <= dot)) return false;
    for (int k = 0; k < K; ++k)
        if (geo_blocked(geo_box(s, k), s.px, s.py, hx, hy)) return false;
    return true;
}

// The field towards the waypoint of an episode that has just begun, one env per 64-thread workgroup (one wavefront), selected like
// nav2d_geo_build_kernel's.  `states` are records that social_begin has just filled.
__global__ void __launch_bounds__(64)
nav2d_social_build_kernel(Nav2DSocialState* __restrict__ states, const uint8_t* __restrict__ mask, int only_ended, int K) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    Nav2DSocialState& r = states[n];
    if (only_ended && !r.base.ended) return;
    __shared__ GeoGraph G;
    geo_graph_nodes(G, r.base, K, lane);
    __syncthreads();
    geo_graph_weights(G, K, lane);
    const float wx = r.wx, wy = r.wy;
    __syncthreads();
    float Dl;
    const int sweeps = geo_field_towards(G, K, wx, wy, lane, Dl);
    if (lane < GEO_NODES) r.DW[lane] = Dl;
    if (lane == 0) r.sweeps = sweeps;
}

// One step of one env by one wavefront (a 64-thread workgroup), as nav2d_rearr_geo_step_kernel.  Every lane takes its own MoveLane
// -- before lane 0 writes any of the record -- and derives the agent's move on it, from the same loads, so the outcome is uniform
// over the wave.  The person's hop is the arg-min form of geo_query_wave: node l with DW[l] on lane l < 32, the waypoint on
// lane 32, and a reduction over (value, rank) with rank 0 for the waypoint and l + 1 for node l, so that among equal values the
// waypoint wins, then the lowest node; the order is total, so every lane ends with the same pair.  A node at distance exactly 0 is
// no candidate.  A waypoint reached or given up draws the next one and builds its field here, the weights included; a step that
// builds nothing needs nodes and boxes alone.  Lane 0 then writes the record back and does the end of the step.  The field of an
// episode that begins here is built by the launch of nav2d_social_build_kernel that follows (only_ended).
__global__ void __launch_bounds__(64)
nav2d_social_step_kernel(Nav2DSocialState* __restrict__ states, const float* __restrict__ dirs, const float* __restrict__ actions,
                         const uint8_t* __restrict__ mask, float* __restrict__ person_sensor, float* __restrict__ person_visible,
                         float* __restrict__ reward, uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed,
                         uint32_t env_offset, int N, int K, int nh, int max_steps, int max_turn, int stop_turn, float min_lin, int sliding,
                         float speed, int always_visible, int advance) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[n]) return;
    Nav2DSocialState& rec = states[n];
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        if (lane == 0) {
            first_episode<false>(rec.base, seed, env, K, nh);
            social_begin(rec, seed, env, K);
        }
    } else {
        __shared__ GeoGraph G;
        MoveLane s = load_move(rec.base);  // this lane's copy
        float hx = rec.obj[0][0], hy = rec.obj[0][1], wx = rec.wx, wy = rec.wy;
        int wp = rec.wp_index;
        float Dl = lane < GEO_NODES ? rec.DW[lane] : INFINITY;
        const uint32_t kw = stream_key(seed, S_WAYPOINT, env, (uint32_t)rec.base.episode);
        // 1. the agent, against the person's old position
        const float a_lin = actions[2 * (size_t)n], a_ang = actions[2 * (size_t)n + 1];
        float l;
        int dh;
        const bool stop = vel_decode(a_lin, a_ang, max_turn, stop_turn, min_lin, l, dh);
        if (!stop)
            vel_move(s, dirs, l, dh, nh, sliding,
                     [&](float x, float y) { return is_free(x, y, rec.base, K) && !(dist(x, y, hx, hy) < OBJ_BLOCK); });
        // 2. the person, against the agent's new position
        geo_graph_nodes(G, rec.base, K, lane);
        __syncthreads();
        float v = INFINITY;
        int rank = lane == GEO_NODES ? 0 : lane + 1;
        if (lane < GEO_NODES) {
            if (Dl < INFINITY && geo_visible(G.boxes, K, hx, hy, G.node_x[lane], G.node_y[lane])) {
                const float di = dist(hx, hy, G.node_x[lane], G.node_y[lane]);
                if (di != 0.0f) v = di + Dl;
            }
        } else if (lane == GEO_NODES) {
            if (geo_visible(G.boxes, K, hx, hy, wx, wy)) v = dist(hx, hy, wx, wy);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o);
            const int orank = __shfl_xor(rank, o);
            if (ov < v || (ov == v && orank < rank)) { v = ov; rank = orank; }
        }
        const bool lost = !(v < INFINITY);
        bool waits = false, arrived = false;
        if (!lost) {
            const int node = rank > 0 ? rank - 1 : 0;  // in 0..31: the minimum is finite, so its rank is at most 32
            const float tx = rank == 0 ? wx : G.node_x[node], ty = rank == 0 ? wy : G.node_y[node];
            const float L = dist(hx, hy, tx, ty);
            float qx = tx, qy = ty;
            if (!(L <= speed)) {
                const float f = __fdiv_rn(speed, L);
                qx = hx + f * (tx - hx); qy = hy + f * (ty - hy);
            }
            if (dist(qx, qy, s.px, s.py) < OBJ_BLOCK) {
                waits = true;
            } else {
                hx = qx; hy = qy;
                arrived = hx == wx && hy == wy;
            }
        }
        const bool rebuild = lost || arrived;  // uniform over the wave, like everything above
        int sweeps = 0;
        if (rebuild) {
            wp += 1;
            social_waypoint(rec.base, kw, K, wp, hx, hy, wx, wy);
            geo_graph_weights(G, K, lane);
            __syncthreads();
            sweeps = geo_field_towards(G, K, wx, wy, lane, Dl);
        }
        __syncthreads();  // every lane has read the record before a lane writes to it
        if (rebuild && lane < GEO_NODES) rec.DW[lane] = Dl;
        if (lane == 0) {
            Nav2DState& t = rec.base;
            store_move(t, s);
            rec.obj[0][0] = hx; rec.obj[0][1] = hy;
            rec.wx = wx; rec.wy = wy; rec.wp_index = wp;
            if (arrived) rec.arrivals += 1;
            if (waits) rec.person_waits += 1;
            if (lost) rec.person_lost += 1;
            if (rebuild) { rec.sweeps = sweeps; rec.rebuilds += 1; }
            // 3. - 5. the terms, the reward, the end of the episode
            float dot, cross;
            const bool sees = social_sees(rec, dirs, K, dot, cross);
            const float d = dist(t.px, t.py, hx, hy);
            const bool following = d >= SOCIAL_NEAR && d <= SOCIAL_FAR && sees;
            const bool was_found = rec.found != 0, sets = following && !was_found;
            reward[n] = ((-0.01f + (t.d_prev - d) * (was_found ? 0.0f : 1.0f)) + (sets ? 2.5f : 0.0f)) + (following ? 0.1f : 0.0f);
            t.d_prev = d;
            t.steps += 1;
            if (sets) { rec.found = 1; rec.first_encounter = t.steps; }
            if (following) rec.following_steps += 1;
            const bool done = t.steps >= max_steps;
            not_done[n] = done ? 0 : 1;
            t.ended = done ? 1 : 0;
            if (done) {
                close_episode<false>(t, (float)rec.found, __fdiv_rn((float)rec.following_steps, (float)t.steps),
                                     (float)(rec.found ? rec.first_encounter : t.steps), (float)t.collisions, sums, seed, env, n, N, K, nh);
                social_begin(rec, seed, env, K);
            }
        }
    }
    if (lane == 0 && (person_sensor || person_visible)) {
        float dot, cross;
        const bool shown = social_sees(rec, dirs, K, dot, cross) || always_visible;
        if (person_sensor) {
            person_sensor[2 * (size_t)n + 0] = shown ? dot : 0.0f;
            person_sensor[2 * (size_t)n + 1] = shown ? cross : 0.0f;
        }
        if (person_visible) person_visible[n] = shown ? 1.0f : 0.0f;
    }
}

// ---- Nav2DExplore-v0 (Nav2DExploreVectorEnv; specification: tests/nav2d_explore_reference.py) ----------------------------------------
// One env of Nav2DExplore-v0: a Nav2D-v0 record (no goal: gx, gy, d_prev and d_start are zero), then the start pose the gps / compass
// sensors refer to, the unoccupied cells of the episode's world, the cells seen so far and the cells the last step saw first.
struct Nav2DExploreState {
    Nav2DState base;
    float sx, sy;
    int32_t h0, free_cells, seen_cells, last_new;
};
static_assert(sizeof(Nav2DExploreState) == HAB_NAV2D_EXPLORE_STATE_BYTES && offsetof(Nav2DExploreState, base) == 0, "Nav2DExploreState layout");
static_assert(offsetof(Nav2DExploreState, sx) == 4 * HAB_NAV2D_EXPLORE_W_START_X && offsetof(Nav2DExploreState, sy) == 4 * HAB_NAV2D_EXPLORE_W_START_Y,
              "Nav2DExploreState layout");
static_assert(offsetof(Nav2DExploreState, h0) == 4 * HAB_NAV2D_EXPLORE_W_START_HEADING &&
              offsetof(Nav2DExploreState, free_cells) == 4 * HAB_NAV2D_EXPLORE_W_FREE_CELLS, "Nav2DExploreState layout");
static_assert(offsetof(Nav2DExploreState, seen_cells) == 4 * HAB_NAV2D_EXPLORE_W_SEEN_CELLS &&
              offsetof(Nav2DExploreState, last_new) == 4 * HAB_NAV2D_EXPLORE_W_LAST_NEW, "Nav2DExploreState layout");

constexpr int EXPLORE_THREADS = 1024;  // one workgroup per env has to fill a CU by itself, as the map's update
constexpr int EXPLORE_WAVES = EXPLORE_THREADS / 64;

// The pose and the rectangles of the record as the sight rule reads them.
__device__ inline void explore_load_sight(nav2d_seen::Sight& e, const Nav2DState& s, const float* __restrict__ dirs, int K) {
    e.px = s.px;
    e.py = s.py;
    e.c = dirs[2 * s.heading];
    e.s = dirs[2 * s.heading + 1];
    for (int k = 0; k < K; ++k) nav2d_seen::set_rect(e, k, s.rect[k][0], s.rect[k][1], s.rect[k][2], s.rect[k][3]);
}

// The sum of `v` over the workgroup, on thread 0: the waves by lane exchange, then the waves' sums through `part`.  Integer, so exact
// and independent of the order.  Ends behind a barrier, so that another sum may follow.
__device__ inline int explore_block_sum(int v, int* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    int total = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < EXPLORE_WAVES; ++w) total += part[w];
    __syncthreads();
    return total;
}

// The range of cell indices along one axis whose centres (i + 0.5) * cell can lie within `vis` of the coordinate p, widened by a
// whole cell on either side.  The rule accepts a centre only if fl(dx * dx) <= fl(vis * vis), so |dx| exceeds vis by a few units
// in the last place at the most, and this arithmetic (inv = G / 8 is 1 / cell to one rounding) is off by less than a thousandth of a
// cell: the margin keeps every cell the rule can accept, so the restricted sweep writes what the full one would.
__device__ inline void explore_axis_range(float p, float vis, float inv, int G, int& lo, int& hi) {
    const float top = (float)(G - 1);
    lo = (int)fminf(fmaxf(floorf((p - vis) * inv) - 1.0f, 0.0f), top);
    hi = (int)fminf(fmaxf(floorf((p + vis) * inv) + 1.0f, 0.0f), top);
}

// One sweep of an env's layer by the workgroup; a thread takes groups of four consecutive cells (one 32-bit word where `vec`).
// BEGIN: the layer is cleared, every cell is visited, `n_free` counts the unoccupied centres and `n_new` the cells of the first
// reveal.  Otherwise only the words of the rows, and in them the columns, of the visibility disc's bounding box are visited, a word
// is written where it changed, and `n_new` counts the cells that turned from 0 to 1.
template <bool BEGIN>
__device__ inline void explore_sweep(uint8_t* __restrict__ layer, const nav2d_seen::Sight& e, int G, int K, float cell, float vis,
                                     float vis2, int vec, int& n_new, int& n_free) {
    const int total = G * G;
    int g_lo = 0, g_hi = (total + 3) >> 2, c_lo = 0, c_hi = G - 1;
    if constexpr (!BEGIN) {
        const float inv = (float)G * 0.125f;
        int j_lo, j_hi;  // y indices: row r has the y index G - 1 - r
        explore_axis_range(e.px, vis, inv, G, c_lo, c_hi);
        explore_axis_range(e.py, vis, inv, G, j_lo, j_hi);
        g_lo = ((G - 1 - j_hi) * G) >> 2;
        g_hi = ((G - j_lo) * G + 3) >> 2;
    }
    for (int g = g_lo + (int)threadIdx.x; g < g_hi; g += EXPLORE_THREADS) {
        const int i0 = g * 4, n = min(4, total - i0);
        uint32_t fv = 0;
        if constexpr (!BEGIN) {
            if (vec) fv = ((const uint32_t*)layer)[g];
            else
                for (int j = 0; j < n; ++j) fv |= (uint32_t)layer[i0 + j] << (8 * j);
        }
        int rr = i0 / G, cc = i0 - rr * G;
        uint32_t fo = fv;
        for (int j = 0; j < n; ++j) {
            if (BEGIN || (!((fv >> (8 * j)) & 255u) && cc >= c_lo && cc <= c_hi)) {
                const float x = ((float)cc + nav2d_seen::HALF) * cell, y = ((float)(G - 1 - rr) + nav2d_seen::HALF) * cell;
                if constexpr (BEGIN) n_free += nav2d_seen::occupied(x, y, e, K) ? 0 : 1;
                if (nav2d_seen::seen_from(x, y, e, K, vis2)) { fo |= 1u << (8 * j); n_new += 1; }
            }
            if (++cc == G) { cc = 0; ++rr; }
        }
        if (BEGIN || fo != fv) {
            if (vec) ((uint32_t*)layer)[g] = fo;
            else
                for (int j = 0; j < n; ++j) layer[i0 + j] = (uint8_t)(fo >> (8 * j));
        }
    }
}

// One workgroup per env, selected by `mask` (NULL: all): an env must not be split, because every thread reads the pose that thread 0
// advances.  Thread 0 moves the agent in the record and puts pose and rectangles into LDS; behind the barrier all threads reveal from
// the new pose and count the new cells; thread 0 ends the step and, where the episode ends, generates the next world; behind another
// barrier the workgroup clears the layer, counts the free cells and does the first reveal.  advance = 0: episode 0, then that last part.
__global__ void __launch_bounds__(EXPLORE_THREADS)
nav2d_explore_step_kernel(Nav2DExploreState* __restrict__ states, const float* __restrict__ dirs, const float* __restrict__ ctab,
                          const int64_t* __restrict__ actions, const uint8_t* __restrict__ mask, float* __restrict__ gps,
                          float* __restrict__ compass, uint8_t* __restrict__ coverage, float* __restrict__ reward,
                          uint8_t* __restrict__ not_done, float* __restrict__ sums, uint32_t seed, uint32_t env_offset, int N, int K, int nh,
                          int max_steps, int G, float cell, float vis, float vis2, float rc, int advance, int vec) {
    const int n = blockIdx.x, tid = threadIdx.x;
    if (mask && !mask[n]) return;
    Nav2DExploreState& o = states[n];
    Nav2DState& s = o.base;
    const uint32_t env = env_offset + (uint32_t)n;
    uint8_t* layer = coverage + (size_t)n * G * G;
    __shared__ nav2d_seen::Sight e;
    __shared__ int part[EXPLORE_WAVES];
    __shared__ int ended;
    if (tid == 0) {
        if (!advance) {
            first_episode<false>(s, seed, env, K, nh);
            s.gx = s.gy = 0.0f;
            s.d_start = s.d_prev = 0.0f;
            o.last_new = 0;
        } else {
            // anything outside 0..3 moves nothing (the host-side entry points refuse it)
            discrete_move(s, actions[n], dirs, nh, [&](float x, float y) { return is_free(x, y, s, K); });
        }
        explore_load_sight(e, s, dirs, K);
    }
    __syncthreads();
    bool begin = !advance;  // uniform over the workgroup, here and after the step
    int n_new = 0, n_free = 0;
    if (advance) {
        explore_sweep<false>(layer, e, G, K, cell, vis, vis2, vec, n_new, n_free);
        const int fresh = explore_block_sum(n_new, part);
        if (tid == 0) {
            reward[n] = -0.01f + rc * (float)fresh;
            o.seen_cells += fresh;
            o.last_new = fresh;
            s.steps += 1;
            const bool done = actions[n] == 0 || s.steps >= max_steps;
            not_done[n] = done ? 0 : 1;
            s.ended = done ? 1 : 0;
            if (done) {
                close_episode<false>(s, __fdiv_rn((float)o.seen_cells, (float)o.free_cells), (cell * cell) * (float)o.seen_cells,
                                     (float)s.collisions, (float)s.steps, sums, seed, env, n, N, K, nh);
                explore_load_sight(e, s, dirs, K);
            }
            ended = done ? 1 : 0;
        }
        __syncthreads();
        begin = ended != 0;
    }
    if (begin) {
        n_new = n_free = 0;
        explore_sweep<true>(layer, e, G, K, cell, vis, vis2, vec, n_new, n_free);
        const int first = explore_block_sum(n_new, part), free_cells = explore_block_sum(n_free, part);
        if (tid == 0) {
            o.sx = s.px; o.sy = s.py; o.h0 = s.heading;
            o.free_cells = free_cells;
            o.seen_cells = first;
        }
    }
    if (tid == 0) {  // Nav2DObj-v0's gps and compass
        if (gps) {
            const float c = dirs[2 * o.h0], sn = dirs[2 * o.h0 + 1];
            to_frame(s.px - o.sx, s.py - o.sy, c, sn, gps[2 * n + 0], gps[2 * n + 1]);
        }
        if (compass) compass[n] = ctab[(s.heading - o.h0 + nh) % nh];
    }
}

// ---- Nav2DImageNav-v0 (Nav2DImageNavVectorEnv; specification: tests/nav2d_imagenav_reference.py) -------------------------------------
// One env of Nav2DImageNav-v0: a Nav2D-v0 record, then the heading the goal image is taken with and the start pose the gps / compass
// sensors refer to.
struct Nav2DImageNavState {
    Nav2DState base;
    int32_t gh;
    float sx, sy;
    int32_t h0;
};
static_assert(sizeof(Nav2DImageNavState) == HAB_NAV2D_IMAGENAV_STATE_BYTES && offsetof(Nav2DImageNavState, base) == 0,
              "Nav2DImageNavState layout");
static_assert(offsetof(Nav2DImageNavState, gh) == 4 * HAB_NAV2D_IMAGENAV_W_GOAL_HEADING &&
              offsetof(Nav2DImageNavState, sx) == 4 * HAB_NAV2D_IMAGENAV_W_START_X, "Nav2DImageNavState layout");
static_assert(offsetof(Nav2DImageNavState, sy) == 4 * HAB_NAV2D_IMAGENAV_W_START_Y &&
              offsetof(Nav2DImageNavState, h0) == 4 * HAB_NAV2D_IMAGENAV_W_START_HEADING, "Nav2DImageNavState layout");

constexpr uint32_t S_GOAL_HEAD = 25u;

// What an episode of Nav2DImageNav-v0 has beyond its Nav2D-v0 world: the goal heading (the start heading's expression on its own
// stream) and the start pose.
__device__ inline void imagenav_begin(Nav2DImageNavState& o, uint32_t seed, uint32_t env, int nh) {
    const Nav2DState& s = o.base;
    o.gh = (int32_t)(mix32(stream_key(seed, S_GOAL_HEAD, env, (uint32_t)s.episode) ^ 0u) % (uint32_t)nh);
    o.sx = s.px; o.sy = s.py; o.h0 = s.heading;
}

// nav2d_step_kernel on such records, with the task's success distance; then Nav2DObj-v0's gps and compass in place of the goal sensor.
template <bool GEO>
__global__ void __launch_bounds__(GEO ? 64 : 1024)
nav2d_imagenav_step_kernel(Nav2DImageNavState* __restrict__ states, const float* __restrict__ dirs, const float* __restrict__ ctab,
                           const int64_t* __restrict__ actions, const uint8_t* __restrict__ mask, float* __restrict__ gps,
                           float* __restrict__ compass, float* __restrict__ reward, uint8_t* __restrict__ not_done,
                           float* __restrict__ sums, uint32_t seed, uint32_t env_offset, int N, int K, int nh, int max_steps,
                           float success_dist, int advance, GeoField* __restrict__ geo) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (mask && !mask[n])) return;
    Nav2DImageNavState& o = states[n];
    Nav2DState& s = o.base;
    const uint32_t env = env_offset + (uint32_t)n;
    if (!advance) {
        first_episode(s, seed, env, K, nh);
        imagenav_begin(o, seed, env, nh);
    } else {
        const int64_t a = actions[n];  // anything outside 0..3 moves nothing (the host-side entry points refuse it)
        discrete_move(s, a, dirs, nh, [&](float x, float y) { return is_free(x, y, s, K); });
        end_step<true, GEO>(s, a == 0, success_dist, reward, not_done, sums, seed, env, n, N, K, nh, max_steps, GEO ? geo + n : nullptr);
        if (s.ended) imagenav_begin(o, seed, env, nh);
    }
    if (gps) {
        const float c = dirs[2 * o.h0], sn = dirs[2 * o.h0 + 1];
        to_frame(s.px - o.sx, s.py - o.sy, c, sn, gps[2 * n + 0], gps[2 * n + 1]);
    }
    if (compass) compass[n] = ctab[(s.heading - o.h0 + nh) % nh];
}

// ---- rendering ---------------------------------------------------------------------------------------------------------------
// Entry / exit of the ray p + t d through [lo, hi] on one axis.
__device__ inline void slab(float lo, float hi, float p, float d, float inv, float& tmin, float& tmax) {
    if (d == 0.0f) {
        const bool inside = p > lo && p < hi;
        tmin = inside ? -INFINITY : INFINITY;
        tmax = inside ? INFINITY : -INFINITY;
        return;
    }
    const float t0 = (lo - p) * inv, t1 = (hi - p) * inv;
    tmin = fminf(t0, t1);
    tmax = fmaxf(t0, t1);
}
__device__ inline uint32_t shade(uint32_t rgb, float depth01) {
    const float s = 1.0f - depth01;
    const uint32_t r = (uint32_t)((float)(rgb & 255u) * s), g = (uint32_t)((float)((rgb >> 8) & 255u) * s),
                   b = (uint32_t)((float)((rgb >> 16) & 255u) * s);
    return r | (g << 8) | (b << 16);
}
constexpr uint32_t pack_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

struct alignas(4) U32x3 { uint32_t a, b, c; };
// floor / ceiling of one row: z, its depth value, its shaded colour, its semantic id (Nav2DObj-v0; 0 otherwise)
struct alignas(16) RowRec { float z, depth; uint32_t color, sem; };

constexpr int RENDER_THREADS = 256;
constexpr int RENDER_MAX_ROWS = 1024;  // rows of one tile
constexpr uint32_t SEM_FLOOR = 0u, SEM_CEILING = 1u, SEM_WALL = 2u, SEM_RECT = 3u, SEM_OBJECT = 4u;

// The colour of an object of one category, the same in every episode.
__device__ inline uint32_t category_color(int32_t cat) {
    const uint32_t c = mix32(0x0B7EC700u + (uint32_t)cat);
    return (128u + (c & 127u)) | ((128u + ((c >> 8) & 127u)) << 8) | ((128u + ((c >> 16) & 127u)) << 16);
}

__host__ __device__ inline int col_slot(int u) { return u + (u >> 5); }
__host__ __device__ inline int col_pitch(int W) { return (col_slot(W) + 4) & ~3; }  // a multiple of 4: `row` stays 16-byte aligned

// One plane of 4-byte pixels (depth, semantic) of the tile [s_px, e_px): pixel (v, u) is wall[col_slot(u)] where the column's hit is
// no farther than the row's floor / ceiling, else flat(row).  Groups of four pixels are one aligned 16-byte store; the up to three
// pixels before the first and after the last group are written one by one.
template <class T, class Flat>
__device__ inline void sweep_dwords(T* __restrict__ img, int s_px, int e_px, int W, int v0, const float* __restrict__ c_z,
                                    const T* __restrict__ wall, const RowRec* __restrict__ row, Flat flat) {
    struct alignas(16) T4 { T x, y, z, w; };
    // first pixel i >= s_px whose address is 16-byte aligned
    const int mis = (int)(((uintptr_t)(img + s_px) >> 2) & 3);
    const int first = min(e_px, s_px + ((4 - mis) & 3));
    const int groups = (e_px - first) >> 2, last = first + (groups << 2);
    for (int g = threadIdx.x; g < groups; g += RENDER_THREADS) {
        const int i = first + (g << 2);
        int v = i / W, u = i - v * W;
        T o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = col_slot(u);
            const RowRec rv = row[v - v0];
            o[j] = c_z[q] <= rv.z ? wall[q] : flat(rv);
            if (++u == W) { u = 0; ++v; }
        }
        *reinterpret_cast<T4*>(img + i) = T4{o[0], o[1], o[2], o[3]};
    }
    const int edge = (first - s_px) + (e_px - last);
    if ((int)threadIdx.x < edge) {
        const int i = (int)threadIdx.x < first - s_px ? s_px + (int)threadIdx.x : last + ((int)threadIdx.x - (first - s_px));
        const int v = i / W, u = i - v * W;
        const int q = col_slot(u);
        const RowRec rv = row[v - v0];
        img[i] = c_z[q] <= rv.z ? wall[q] : flat(rv);
    }
}

// grid (row tiles, N), RENDER_THREADS threads.  Phase 1: the W column hits and the tile's row constants, once per workgroup, into
// LDS.  Phase 2: the tile's pixels are one contiguous range of the image; it is swept in groups of four pixels placed so that the
// depth group is one aligned 16-byte store and the rgb group three whole dwords; the up to three pixels before the first and
// after the last group are written one by one.
// LDS: four per-column arrays (z_wall, depth of the wall, z seen by rgb, shaded wall colour) and row[r] = (z of floor / ceiling, its
// depth, its shaded colour, as a RowRec).  Colours are packed integers and stay uint32_t from LDS to the store.  A lane's four pixels
// are four consecutive columns, so the lanes of a wave read the column arrays at a stride of four dwords; column u sits at
// u + (u >> 5), which spreads a half wave's 32 reads over the 32 banks.
// Render::OBJ (Nav2DObj-v0): `states` are Nav2DObjState records; the M cylinders are geometry that depth, rgb and semantic see alike
// and there is no goal marker; a fifth per-column array holds the semantic id of the column's hit and a third sweep writes `semantic`
// like depth.  LDS is (4 or 5) * col_pitch(W) dwords + 16 bytes per tile row: at most 20 * 2116 + 16 * 4 bytes (W = 2048) or
// 16 * 1024 + 20 * 4 (W = 1), under 64 KiB for every accepted width.
// Render::REARR (Nav2DRearr-v0): `states` are Nav2DRearrState records; the object is one cylinder of category 0's colour, geometry
// for depth and rgb alike while the env's holding flag is clear and absent while it is set; the goal marker is drawn in rgb as in
// the GOAL form, nearer than whatever the column hit, the cylinder included.  No semantic image: four column arrays.
// Render::SOCIAL (Nav2DSocial-v0): `states` are Nav2DSocialState records; the person is one cylinder of category 0's colour, geometry
// for depth and rgb alike, and there is no goal marker: nothing is drawn in rgb only.  No semantic image: four column arrays.
// Render::EXPLORE (Nav2DExplore-v0): `states` are Nav2DExploreState records; Nav2D-v0's geometry with no cylinder and no goal marker.
// Render::IMAGENAV (Nav2DImageNav-v0): `states` are Nav2DImageNavState records; the EXPLORE form's markerless geometry, drawn twice in
// one launch: grid (row tiles, N, 2), and the third index selects the view, so the choice is uniform over a workgroup.  View 0 is the
// agent's pose into `rgb` / `depth`; view 1 is the pose (gx, gy, gh) of the record into `goal_rgb`, colour only.  A view none of whose
// destinations is given leaves before the first barrier.  `goal_rgb` is read by this form alone.
enum class Render { GOAL, OBJ, REARR, SOCIAL, EXPLORE, IMAGENAV };
template <Render MODE>
__global__ void __launch_bounds__(RENDER_THREADS)
nav2d_render_kernel(const void* __restrict__ states, const float* __restrict__ ray, const float* __restrict__ col_cos,
                    const float* __restrict__ tanv, const uint8_t* __restrict__ mask, uint8_t* __restrict__ rgb,
                    float* __restrict__ depth, int32_t* __restrict__ semantic, int H, int W, int K, int M, int rows_per_tile,
                    uint8_t* __restrict__ goal_rgb) {
    extern __shared__ uint4 lds[];
    const int n = blockIdx.y;
    if (mask && !mask[n]) return;
    constexpr bool IMAGENAV = MODE == Render::IMAGENAV;
    const bool goal_view = IMAGENAV && blockIdx.z == 1;
    if constexpr (IMAGENAV) {
        rgb = goal_view ? goal_rgb : rgb;
        depth = goal_view ? nullptr : depth;
        if (!rgb && !depth) return;
    }
    const int P = col_pitch(W);
    float* c_zd = reinterpret_cast<float*>(lds);
    float* c_dw = c_zd + P;
    float* c_zr = c_dw + P;
    uint32_t* c_cw = reinterpret_cast<uint32_t*>(c_zr + P);
    int32_t* c_sem = reinterpret_cast<int32_t*>(c_cw + P);  // OBJ only
    constexpr bool OBJ = MODE == Render::OBJ, REARR = MODE == Render::REARR, SOCIAL = MODE == Render::SOCIAL, EXPLORE = MODE == Render::EXPLORE;
    RowRec* row = reinterpret_cast<RowRec*>(lds + P) + (OBJ ? P / 4 : 0);
    const Nav2DObjState* os = OBJ ? static_cast<const Nav2DObjState*>(states) + n : nullptr;
    const Nav2DRearrState* rs = REARR ? static_cast<const Nav2DRearrState*>(states) + n : nullptr;
    const Nav2DSocialState* ss = SOCIAL ? static_cast<const Nav2DSocialState*>(states) + n : nullptr;
    const Nav2DExploreState* es = EXPLORE ? static_cast<const Nav2DExploreState*>(states) + n : nullptr;
    const Nav2DImageNavState* is = IMAGENAV ? static_cast<const Nav2DImageNavState*>(states) + n : nullptr;
    const Nav2DState& s = OBJ ? os->base : REARR ? rs->base : SOCIAL ? ss->base : EXPLORE ? es->base : IMAGENAV ? is->base
                                                                                              : static_cast<const Nav2DState*>(states)[n];
    // the cylinders of this env: Nav2DObj-v0's M objects, Nav2DRearr-v0's object unless it is held, Nav2DSocial-v0's person
    const float (*cyl)[2] = OBJ ? os->obj : REARR ? reinterpret_cast<const float (*)[2]>(&rs->ox) : SOCIAL ? ss->obj : nullptr;
    const int cyls = OBJ ? M : REARR ? (rs->holding ? 0 : 1) : SOCIAL ? 1 : 0;
    const int v0 = blockIdx.x * rows_per_tile, v1 = min(H, v0 + rows_per_tile);
    // the camera's pose: the agent's, or for the goal view of the IMAGENAV form the goal position with the goal heading
    const float px = goal_view ? s.gx : s.px, py = goal_view ? s.gy : s.py;
    const float* rayh = ray + (size_t)(goal_view ? is->gh : s.heading) * W * 2;
    for (int u = threadIdx.x; u < W; u += RENDER_THREADS) {
        const float dx = rayh[2 * u], dy = rayh[2 * u + 1];
        const float ix = __fdiv_rn(1.0f, dx), iy = __fdiv_rn(1.0f, dy);
        const float tx = dx > 0.0f ? (ARENA - px) * ix : (dx < 0.0f ? (0.0f - px) * ix : INFINITY);
        const float ty = dy > 0.0f ? (ARENA - py) * iy : (dy < 0.0f ? (0.0f - py) * iy : INFINITY);
        float t = tx <= ty ? tx : ty;
        int hit = tx <= ty ? (dx > 0.0f ? 0 : 1) : (dy > 0.0f ? 2 : 3);
        for (int k = 0; k < K; ++k) {
            float axn, axx, ayn, ayx;
            slab(s.rect[k][0], s.rect[k][2], px, dx, ix, axn, axx);
            slab(s.rect[k][1], s.rect[k][3], py, dy, iy, ayn, ayx);
            const float tn = fmaxf(axn, ayn), tm = fminf(axx, ayx);
            if (tn <= tm && tn > 0.0f && tn < t) { t = tn; hit = 4 + k; }
        }
        if constexpr (OBJ || REARR || SOCIAL) {
            // the cylinders: the goal marker's ray-circle test (nearest intersection, ray direction taken as unit length)
            for (int j = 0; j < cyls; ++j) {
                const float ox = px - cyl[j][0], oy = py - cyl[j][1];
                const float b = ox * dx + oy * dy;
                const float c = (ox * ox + oy * oy) - OBJ_R * OBJ_R;
                const float disc = b * b - c;
                const float to = -b - sqrt_rn(fmaxf(disc, 0.0f));
                if (disc >= 0.0f && to > 0.0f && to < t) { t = to; hit = 4 + MAX_K + j; }
            }
        }
        const float cf = col_cos[u];
        const float z_wall = t * cf;
        float z_rgb = z_wall;
        bool marker = false;
        if constexpr (!OBJ && !SOCIAL && !EXPLORE && !IMAGENAV) {
            const float ox = px - s.gx, oy = py - s.gy;
            const float b = ox * dx + oy * dy;
            const float c = (ox * ox + oy * oy) - 0.2f * 0.2f;
            const float disc = b * b - c;
            const float tmk = -b - sqrt_rn(fmaxf(disc, 0.0f));
            marker = disc >= 0.0f && tmk > 0.0f && tmk < t;
            z_rgb = marker ? tmk * cf : z_wall;
        }
        uint32_t base;
        if (marker) base = pack_rgb(255, 32, 32);
        else if ((OBJ || REARR || SOCIAL) && hit >= 4 + MAX_K) base = category_color(OBJ ? os->cat[hit - (4 + MAX_K)] : 0);
        else if (hit >= 4) base = s.color[hit - 4];
        else base = hit == 0 ? pack_rgb(200, 180, 150) : hit == 1 ? pack_rgb(150, 200, 180) : hit == 2 ? pack_rgb(180, 150, 200)
                                                                                                        : pack_rgb(200, 200, 150);
        const float d_wall = fminf(__fdiv_rn(z_wall, 10.0f), 1.0f), d_rgbw = fminf(__fdiv_rn(z_rgb, 10.0f), 1.0f);
        const int q = col_slot(u);
        c_zd[q] = z_wall;
        c_dw[q] = d_wall;
        c_zr[q] = z_rgb;
        c_cw[q] = shade(base, d_rgbw);
        if constexpr (OBJ)
            c_sem[q] = hit >= 4 + MAX_K ? (int32_t)SEM_OBJECT + os->cat[hit - (4 + MAX_K)] : (int32_t)(hit >= 4 ? SEM_RECT : SEM_WALL);
    }
    for (int r = threadIdx.x; r < v1 - v0; r += RENDER_THREADS) {
        const float tv = tanv[v0 + r];
        const float zf = __fdiv_rn(1.25f, fabsf(tv));
        const float d_flat = fminf(__fdiv_rn(zf, 10.0f), 1.0f);
        row[r] = RowRec{zf, d_flat, shade(tv > 0.0f ? pack_rgb(230, 230, 240) : pack_rgb(110, 100, 90), d_flat),
                        OBJ ? (tv > 0.0f ? SEM_CEILING : SEM_FLOOR) : 0u};
    }
    __syncthreads();

    const long long img = (long long)n * H * W;   // first pixel of this env's image, in pixels from the tensor base
    const int s_px = v0 * W, e_px = v1 * W;       // this tile's pixel range within the image
    if (depth) sweep_dwords(depth + img, s_px, e_px, W, v0, c_zd, c_dw, row, [](const RowRec& rv) { return rv.depth; });
    if (rgb) {
        uint8_t* cimg = rgb + img * 3;
        // first pixel i >= s_px whose byte address is dword aligned: (base + 3 i) % 4 == 0  <=>  i % 4 == base % 4
        const int mis = (int)(((uintptr_t)cimg - (uintptr_t)s_px) & 3);   // (base - s_px) mod 4
        const int first = min(e_px, s_px + mis);
        const int groups = (e_px - first) >> 2, last = first + (groups << 2);
        for (int g = threadIdx.x; g < groups; g += RENDER_THREADS) {
            const int i = first + (g << 2);
            int v = i / W, u = i - v * W;
            uint32_t p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = col_slot(u);
                const RowRec rv = row[v - v0];
                p[j] = c_zr[q] <= rv.z ? c_cw[q] : rv.color;
                if (++u == W) { u = 0; ++v; }
            }
            U32x3 w;
            w.a = p[0] | (p[1] << 24);
            w.b = (p[1] >> 8) | (p[2] << 16);
            w.c = (p[2] >> 16) | (p[3] << 8);
            *reinterpret_cast<U32x3*>(cimg + (size_t)i * 3) = w;
        }
        const int edge = (first - s_px) + (e_px - last);
        if ((int)threadIdx.x < edge) {
            const int i = (int)threadIdx.x < first - s_px ? s_px + (int)threadIdx.x : last + ((int)threadIdx.x - (first - s_px));
            const int v = i / W, u = i - v * W;
            const int q = col_slot(u);
            const RowRec rv = row[v - v0];
            const uint32_t p = c_zr[q] <= rv.z ? c_cw[q] : rv.color;
            cimg[(size_t)i * 3 + 0] = (uint8_t)(p & 255u);
            cimg[(size_t)i * 3 + 1] = (uint8_t)((p >> 8) & 255u);
            cimg[(size_t)i * 3 + 2] = (uint8_t)((p >> 16) & 255u);
        }
    }
    if constexpr (OBJ)
        if (semantic)
            sweep_dwords(semantic + img, s_px, e_px, W, v0, c_zd, c_sem, row, [](const RowRec& rv) { return (int32_t)rv.sem; });
}

}  // namespace nav2d

using namespace nav2d;

extern "C" int hab_nav2d_state_bytes(void) { return (int)sizeof(Nav2DState); }

extern "C" int hab_nav2d_obj_state_bytes(void) { return (int)sizeof(Nav2DObjState); }

// What every step entry is given, in the order of the C signatures.  NULL where the entry has none: `geo`, the field of a `_geo`
// entry; `goal`, the sensor row of the point-goal tasks; `semantic`, Nav2DObj-v0's image.
struct StepArgs {
    void *state, *geo;
    const float *dirs, *ray, *col_cos, *tanv;
    const void* actions;
    const uint8_t* mask;
    uint8_t* rgb;
    float *depth, *goal;
    int32_t* semantic;
    float* reward;
    uint8_t* not_done;
    float* measure_sums;
    uint32_t seed, env_offset;
    int N, H, W, num_obstacles, num_headings, max_episode_steps, advance;
    hipStream_t stream;
    uint8_t* goal_rgb = nullptr;  // Nav2DImageNav-v0's second view
    bool image() const { return rgb || depth || semantic || goal_rgb; }  // whether any image destination is given
};

static int check_geo_args(const void* state, size_t state_stride_bytes, const void* geo, int N, int num_obstacles) {
    if (!state || !geo || ((uintptr_t)geo & 3) || ((uintptr_t)state & 3) || N <= 0) return HAB_ERR_ARG;
    if (state_stride_bytes < sizeof(Nav2DState) || (state_stride_bytes & 3)) return HAB_ERR_ARG;
    if (num_obstacles < 0 || num_obstacles > MAX_K) return HAB_ERR_ARG;
    return HAB_OK;
}

// The argument checks the step entries share, then, for a `_geo` entry, those of the field; `state_stride` is the size of the task's
// state record.
static int check_step_args(const StepArgs& a, bool geo_entry, size_t state_stride = sizeof(Nav2DState)) {
    if (!a.state || !a.dirs || a.N <= 0 || a.num_headings <= 0 || a.max_episode_steps <= 0) return HAB_ERR_ARG;
    if (a.num_obstacles < 0 || a.num_obstacles > MAX_K) return HAB_ERR_ARG;
    if (a.advance && (!a.actions || !a.reward || !a.not_done)) return HAB_ERR_ARG;
    if (a.image() && (!a.ray || !a.col_cos || !a.tanv || a.H <= 0 || a.W <= 0)) return HAB_ERR_ARG;
    if (a.image() && (a.W > HAB_NAV2D_MAX_WIDTH || (long long)a.H * a.W > (1ll << 24))) return HAB_ERR_UNSUPPORTED;
    if (a.image() && a.N > 65535) return HAB_ERR_UNSUPPORTED;  // the render's grid.y is the env
    if (a.depth && ((uintptr_t)a.depth & 3)) return HAB_ERR_ARG;
    return geo_entry ? check_geo_args(a.state, state_stride, a.geo, a.N, a.num_obstacles) : HAB_OK;
}

// The motion parameters of the velocity tasks.
static bool vel_args_ok(int max_turn_steps, int stop_turn_steps, int num_headings) {
    return max_turn_steps >= 1 && max_turn_steps <= num_headings / 2 && stop_turn_steps >= 1 && stop_turn_steps <= max_turn_steps;
}
static bool start_holding_ok(int start_holding) { return start_holding == 0 || start_holding == 1; }
// What the follower and the oracle are given beside state and field; an action row is read and written as one word of its size.
static bool guide_args_ok(const float* dirs, const void* actions, size_t action_bytes, const float* next_d, const int32_t* status,
                          int num_headings) {
    if (!dirs || ((uintptr_t)dirs & 3) || !actions || ((uintptr_t)actions & (action_bytes - 1))) return false;
    return !((uintptr_t)next_d & 3) && !((uintptr_t)status & 3) && num_headings > 0;
}

// The render, where an image destination is given, in the task's form.  `semantic` and `num_objects` are used by the Nav2DObj-v0
// instantiation alone.
template <Render MODE>
static int launch_render(const StepArgs& a, int num_objects) {
    if (!a.image()) return HAB_OK;
    // a tile is at least ~16 KiB of stores per workgroup, so that the W column hits are a small part of its work
    // and at most RENDER_MAX_ROWS, which keeps the dynamic LDS below 64 KiB for every accepted W
    int rows = cdiv(4096, a.W);
    if (rows < 4) rows = 4;
    if (rows > RENDER_MAX_ROWS) rows = RENDER_MAX_ROWS;
    if (rows > a.H) rows = a.H;
    dim3 grid(cdiv(a.H, rows), a.N, MODE == Render::IMAGENAV ? 2 : 1);
    const size_t lds = (size_t)(col_pitch(a.W) + rows) * sizeof(uint4) +
                       (MODE == Render::OBJ ? (size_t)col_pitch(a.W) * sizeof(int32_t) : 0);
    nav2d_render_kernel<MODE><<<grid, RENDER_THREADS, lds, a.stream>>>(a.state, a.ray, a.col_cos, a.tanv, a.mask, a.rgb, a.depth, a.semantic,
                                                                       a.H, a.W, a.num_obstacles, num_objects, rows, a.goal_rgb);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

// What follows the step kernel of a point-goal task: for a `_geo` entry the fields of the episodes that began (at a reset, of every
// env the mask selects), then the render.
template <bool GEO>
static int finish_goal_step(const StepArgs& a) {
    if (GEO) {
        nav2d_geo_build_kernel<<<a.N, 64, 0, a.stream>>>((char*)a.state, sizeof(Nav2DState), (GeoField*)a.geo, a.mask, a.advance ? 1 : 0,
                                                         a.num_obstacles);
        HAB_LAUNCH_CHECK();
    }
    return launch_render<Render::GOAL>(a, 0);
}

// Nav2D-v0.  hab_nav2d_step is <false> with geo = NULL, which is what its kernel is given; hab_nav2d_step_geo is <true>.
template <bool GEO>
static int step(const StepArgs& a) {
    const int rc = check_step_args(a, GEO);
    if (rc != HAB_OK) return rc;
    nav2d_step_kernel<GEO><<<cdiv(a.N, 64), 64, 0, a.stream>>>((Nav2DState*)a.state, a.dirs, (const int64_t*)a.actions, a.mask, a.goal,
                                                                a.reward, a.not_done, a.measure_sums, a.seed, a.env_offset, a.N,
                                                                a.num_obstacles, a.num_headings, a.max_episode_steps, a.advance,
                                                                GEO ? (GeoField*)a.geo : nullptr);
    HAB_LAUNCH_CHECK();
    return finish_goal_step<GEO>(a);
}

extern "C" int hab_nav2d_step(void* state, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                              const int64_t* actions, const uint8_t* mask, uint8_t* rgb, float* depth, float* goal, float* reward,
                              uint8_t* not_done, float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H, int W,
                              int num_obstacles, int num_headings, int max_episode_steps, int advance, hipStream_t stream) {
    return step<false>({state, nullptr, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, goal, nullptr, reward, not_done, measure_sums,
                        seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream});
}

extern "C" int hab_nav2d_step_geo(void* state, void* geo, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                  const int64_t* actions, const uint8_t* mask, uint8_t* rgb, float* depth, float* goal, float* reward,
                                  uint8_t* not_done, float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H, int W,
                                  int num_obstacles, int num_headings, int max_episode_steps, int advance, hipStream_t stream) {
    return step<true>({state, geo, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, goal, nullptr, reward, not_done, measure_sums,
                       seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream});
}

extern "C" int hab_nav2d_geo_bytes(void) { return (int)sizeof(GeoField); }

extern "C" int hab_nav2d_geo_build(void* state, size_t state_stride_bytes, void* geo, const uint8_t* mask, int only_ended, int N,
                                   int num_obstacles, hipStream_t stream) {
    const int rc = check_geo_args(state, state_stride_bytes, geo, N, num_obstacles);
    if (rc != HAB_OK) return rc;
    nav2d_geo_build_kernel<<<N, 64, 0, stream>>>((char*)state, state_stride_bytes, (GeoField*)geo, mask, only_ended, num_obstacles);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

// Nav2DVel-v0, its two entries like Nav2D-v0's.
template <bool GEO>
static int vel_step(const StepArgs& a, int max_turn_steps, int stop_turn_steps, float min_abs_lin_speed, int allow_sliding) {
    const int rc = check_step_args(a, GEO);
    if (rc != HAB_OK) return rc;
    if ((uintptr_t)a.actions & 7) return HAB_ERR_ARG;  // a row is read as one float2
    if (!vel_args_ok(max_turn_steps, stop_turn_steps, a.num_headings)) return HAB_ERR_ARG;
    nav2d_vel_step_kernel<GEO><<<cdiv(a.N, 64), 64, 0, a.stream>>>((Nav2DState*)a.state, a.dirs, (const float2*)a.actions, a.mask, a.goal,
                                                                    a.reward, a.not_done, a.measure_sums, a.seed, a.env_offset, a.N,
                                                                    a.num_obstacles, a.num_headings, a.max_episode_steps, max_turn_steps,
                                                                    stop_turn_steps, min_abs_lin_speed, allow_sliding, a.advance,
                                                                    GEO ? (GeoField*)a.geo : nullptr);
    HAB_LAUNCH_CHECK();
    return finish_goal_step<GEO>(a);
}

extern "C" int hab_nav2d_vel_step(void* state, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                  const float* actions, const uint8_t* mask, uint8_t* rgb, float* depth, float* goal, float* reward,
                                  uint8_t* not_done, float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H, int W,
                                  int num_obstacles, int num_headings, int max_episode_steps, int max_turn_steps, int stop_turn_steps,
                                  float min_abs_lin_speed, int allow_sliding, int advance, hipStream_t stream) {
    return vel_step<false>({state, nullptr, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, goal, nullptr, reward, not_done,
                            measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream},
                           max_turn_steps, stop_turn_steps, min_abs_lin_speed, allow_sliding);
}

extern "C" int hab_nav2d_vel_step_geo(void* state, void* geo, const float* dirs, const float* ray, const float* col_cos,
                                      const float* tanv, const float* actions, const uint8_t* mask, uint8_t* rgb, float* depth,
                                      float* goal, float* reward, uint8_t* not_done, float* measure_sums, uint32_t seed,
                                      uint32_t env_offset, int N, int H, int W, int num_obstacles, int num_headings,
                                      int max_episode_steps, int max_turn_steps, int stop_turn_steps, float min_abs_lin_speed,
                                      int allow_sliding, int advance, hipStream_t stream) {
    return vel_step<true>({state, geo, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, goal, nullptr, reward, not_done, measure_sums,
                           seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream},
                          max_turn_steps, stop_turn_steps, min_abs_lin_speed, allow_sliding);
}

// The shortest-path follower: the checks of the field entries, then those of its own arguments.
template <class Writer>
static int follow(const void* state, size_t state_stride_bytes, const void* geo, const float* dirs, const uint8_t* mask,
                  typename Writer::Action* actions, float* next_d, int32_t* status, int N, int num_obstacles, int num_headings,
                  hipStream_t stream, Writer writer) {
    const int rc = check_geo_args(state, state_stride_bytes, geo, N, num_obstacles);
    if (rc != HAB_OK) return rc;
    if (!guide_args_ok(dirs, actions, sizeof(typename Writer::Action), next_d, status, num_headings)) return HAB_ERR_ARG;
    nav2d_follow_kernel<Writer><<<N, 64, 0, stream>>>((const char*)state, state_stride_bytes, (const GeoField*)geo, dirs, mask, actions,
                                                      next_d, status, num_obstacles, num_headings, writer);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

extern "C" int hab_nav2d_follow(const void* state, size_t state_stride_bytes, const void* geo, const float* dirs, const uint8_t* mask,
                                int64_t* actions, float* next_d, int32_t* status, int N, int num_obstacles, int num_headings,
                                hipStream_t stream) {
    return follow(state, state_stride_bytes, geo, dirs, mask, actions, next_d, status, N, num_obstacles, num_headings, stream,
                  FollowDiscrete{});
}

extern "C" int hab_nav2d_vel_follow(const void* state, size_t state_stride_bytes, const void* geo, const float* dirs,
                                    const uint8_t* mask, float* actions, float* next_d, int32_t* status, int N, int num_obstacles,
                                    int num_headings, int max_turn_steps, hipStream_t stream) {
    if (num_headings <= 0 || max_turn_steps < 1 || max_turn_steps > num_headings / 2) return HAB_ERR_ARG;
    return follow(state, state_stride_bytes, geo, dirs, mask, (float2*)actions, next_d, status, N, num_obstacles, num_headings, stream,
                  FollowVelocity{max_turn_steps});
}

// Nav2DObj-v0, its two entries like Nav2D-v0's.  GEO: the step is one wavefront per env, and the fields of the episodes that began (at
// a reset, of every env the mask selects) follow it.
template <bool GEO>
static int obj_step(const StepArgs& a, int64_t* objectgoal, float* gps, float* compass, const float* compass_table, int num_objects,
                    int num_categories, int num_actions) {
    const int rc = check_step_args(a, GEO, sizeof(Nav2DObjState));
    if (rc != HAB_OK) return rc;
    if (a.semantic && ((uintptr_t)a.semantic & 3)) return HAB_ERR_ARG;
    if (compass && !compass_table) return HAB_ERR_ARG;
    if (num_objects < 1 || num_objects > MAX_M || num_categories < 1 || num_categories > HAB_NAV2D_MAX_CATEGORIES) return HAB_ERR_ARG;
    if (num_actions != 4 && num_actions != 6) return HAB_ERR_ARG;
    Nav2DObjState* states = (Nav2DObjState*)a.state;
    const int64_t* actions = (const int64_t*)a.actions;
    if constexpr (GEO) {
        nav2d_obj_geo_step_kernel<<<a.N, 64, 0, a.stream>>>(states, (ObjGeoField*)a.geo, a.dirs, compass_table, actions, a.mask, objectgoal, gps,
                                                            compass, a.reward, a.not_done, a.measure_sums, a.seed, a.env_offset, a.N,
                                                            a.num_obstacles, a.num_headings, a.max_episode_steps, num_objects,
                                                            num_categories, a.advance);
        HAB_LAUNCH_CHECK();
        nav2d_obj_geo_build_kernel<<<a.N, 64, 0, a.stream>>>((char*)a.state, sizeof(Nav2DObjState), (ObjGeoField*)a.geo, a.mask,
                                                             a.advance ? 1 : 0, a.num_obstacles, num_objects);
    } else {
        nav2d_obj_step_kernel<<<cdiv(a.N, 64), 64, 0, a.stream>>>(states, a.dirs, compass_table, actions, a.mask, objectgoal, gps, compass,
                                                                  a.reward, a.not_done, a.measure_sums, a.seed, a.env_offset, a.N,
                                                                  a.num_obstacles, a.num_headings, a.max_episode_steps, num_objects,
                                                                  num_categories, a.advance);
    }
    HAB_LAUNCH_CHECK();
    return launch_render<Render::OBJ>(a, num_objects);
}

extern "C" int hab_nav2d_obj_step(void* state, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                  const int64_t* actions, const uint8_t* mask, uint8_t* rgb, float* depth, int32_t* semantic,
                                  int64_t* objectgoal, float* gps, float* compass, const float* compass_table, float* reward,
                                  uint8_t* not_done, float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H, int W,
                                  int num_obstacles, int num_headings, int max_episode_steps, int num_objects, int num_categories,
                                  int num_actions, int advance, hipStream_t stream) {
    return obj_step<false>({state, nullptr, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, nullptr, semantic, reward, not_done,
                            measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream},
                           objectgoal, gps, compass, compass_table, num_objects, num_categories, num_actions);
}

extern "C" int hab_nav2d_obj_step_geo(void* state, void* geo, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                      const int64_t* actions, const uint8_t* mask, uint8_t* rgb, float* depth, int32_t* semantic,
                                      int64_t* objectgoal, float* gps, float* compass, const float* compass_table, float* reward,
                                      uint8_t* not_done, float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H, int W,
                                      int num_obstacles, int num_headings, int max_episode_steps, int num_objects, int num_categories,
                                      int num_actions, int advance, hipStream_t stream) {
    return obj_step<true>({state, geo, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, nullptr, semantic, reward, not_done,
                           measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream},
                          objectgoal, gps, compass, compass_table, num_objects, num_categories, num_actions);
}

extern "C" int hab_nav2d_obj_geo_bytes(void) { return (int)sizeof(ObjGeoField); }

extern "C" int hab_nav2d_obj_geo_build(void* state, size_t state_stride_bytes, void* geo, const uint8_t* mask, int only_ended, int N,
                                       int num_obstacles, int num_objects, hipStream_t stream) {
    const int rc = check_geo_args(state, state_stride_bytes, geo, N, num_obstacles);
    if (rc != HAB_OK) return rc;
    if (state_stride_bytes < sizeof(Nav2DObjState)) return HAB_ERR_ARG;
    if (num_objects < 1 || num_objects > MAX_M) return HAB_ERR_ARG;
    nav2d_obj_geo_build_kernel<<<N, 64, 0, stream>>>((char*)state, state_stride_bytes, (ObjGeoField*)geo, mask, only_ended, num_obstacles,
                                                     num_objects);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

extern "C" int hab_nav2d_rearr_state_bytes(void) { return (int)sizeof(Nav2DRearrState); }

extern "C" int hab_nav2d_rearr_geo_bytes(void) { return (int)sizeof(RearrGeoField); }

extern "C" int hab_nav2d_rearr_geo_build(void* state, size_t state_stride_bytes, void* geo, const uint8_t* mask, int only_ended, int N,
                                         int num_obstacles, int start_holding, hipStream_t stream) {
    const int rc = check_geo_args(state, state_stride_bytes, geo, N, num_obstacles);
    if (rc != HAB_OK) return rc;
    if (state_stride_bytes < sizeof(Nav2DRearrState)) return HAB_ERR_ARG;
    if (!start_holding_ok(start_holding)) return HAB_ERR_ARG;
    nav2d_rearr_geo_build_kernel<<<N, 64, 0, stream>>>((char*)state, state_stride_bytes, (RearrGeoField*)geo, mask, only_ended,
                                                       num_obstacles, start_holding);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

// The four rearrangement steps.  VEL: `actions` are Nav2DRearrVel-v0's (N, 3) float rows and the four motion parameters are used; else
// int64 actions, and the parameters are unused.  GEO: the step is one wavefront per env, and the fields of the episodes that began (at
// a reset, of every env the mask selects) follow it.  Then the render.
template <bool VEL, bool GEO>
static int rearr_step(const StepArgs& a, float* obj_start, float* obj_goal, float* is_holding, int start_holding, int max_turn_steps,
                      int stop_turn_steps, float min_abs_lin_speed, int allow_sliding) {
    const int rc = check_step_args(a, GEO, sizeof(Nav2DRearrState));
    if (rc != HAB_OK) return rc;
    if (!start_holding_ok(start_holding)) return HAB_ERR_ARG;
    if (VEL) {
        if ((uintptr_t)a.actions & 3) return HAB_ERR_ARG;  // a row of three floats is read as three scalars
        if (!vel_args_ok(max_turn_steps, stop_turn_steps, a.num_headings)) return HAB_ERR_ARG;
    }
    Nav2DRearrState* states = (Nav2DRearrState*)a.state;
    if constexpr (GEO) {
        nav2d_rearr_geo_step_kernel<VEL><<<a.N, 64, 0, a.stream>>>(states, (RearrGeoField*)a.geo, a.dirs, a.actions, a.mask, obj_start, obj_goal,
                                                                   is_holding, a.reward, a.not_done, a.measure_sums, a.seed, a.env_offset,
                                                                   a.N, a.num_obstacles, a.num_headings, a.max_episode_steps, start_holding,
                                                                   max_turn_steps, stop_turn_steps, min_abs_lin_speed, allow_sliding,
                                                                   a.advance);
        HAB_LAUNCH_CHECK();
        nav2d_rearr_geo_build_kernel<<<a.N, 64, 0, a.stream>>>((char*)a.state, sizeof(Nav2DRearrState), (RearrGeoField*)a.geo, a.mask,
                                                               a.advance ? 1 : 0, a.num_obstacles, start_holding);
    } else if constexpr (VEL) {
        nav2d_rearr_vel_step_kernel<<<cdiv(a.N, 64), 64, 0, a.stream>>>(states, a.dirs, (const float*)a.actions, a.mask, obj_start, obj_goal,
                                                                        is_holding, a.reward, a.not_done, a.measure_sums, a.seed,
                                                                        a.env_offset, a.N, a.num_obstacles, a.num_headings,
                                                                        a.max_episode_steps, start_holding, max_turn_steps, stop_turn_steps,
                                                                        min_abs_lin_speed, allow_sliding, a.advance);
    } else {
        nav2d_rearr_step_kernel<<<cdiv(a.N, 64), 64, 0, a.stream>>>(states, a.dirs, (const int64_t*)a.actions, a.mask, obj_start, obj_goal,
                                                                    is_holding, a.reward, a.not_done, a.measure_sums, a.seed, a.env_offset,
                                                                    a.N, a.num_obstacles, a.num_headings, a.max_episode_steps, start_holding,
                                                                    a.advance);
    }
    HAB_LAUNCH_CHECK();
    return launch_render<Render::REARR>(a, 0);
}

extern "C" int hab_nav2d_rearr_step(void* state, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                    const int64_t* actions, const uint8_t* mask, uint8_t* head_rgb, float* head_depth, float* obj_start,
                                    float* obj_goal, float* is_holding, float* reward, uint8_t* not_done, float* measure_sums,
                                    uint32_t seed, uint32_t env_offset, int N, int H, int W, int num_obstacles, int num_headings,
                                    int max_episode_steps, int start_holding, int advance, hipStream_t stream) {
    return rearr_step<false, false>({state, nullptr, dirs, ray, col_cos, tanv, actions, mask, head_rgb, head_depth, nullptr, nullptr, reward,
                                     not_done, measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps,
                                     advance, stream},
                                    obj_start, obj_goal, is_holding, start_holding, 0, 0, 0.0f, 0);
}

extern "C" int hab_nav2d_rearr_vel_step(void* state, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                        const float* actions, const uint8_t* mask, uint8_t* head_rgb, float* head_depth, float* obj_start,
                                        float* obj_goal, float* is_holding, float* reward, uint8_t* not_done, float* measure_sums,
                                        uint32_t seed, uint32_t env_offset, int N, int H, int W, int num_obstacles, int num_headings,
                                        int max_episode_steps, int start_holding, int max_turn_steps, int stop_turn_steps,
                                        float min_abs_lin_speed, int allow_sliding, int advance, hipStream_t stream) {
    return rearr_step<true, false>({state, nullptr, dirs, ray, col_cos, tanv, actions, mask, head_rgb, head_depth, nullptr, nullptr, reward,
                                    not_done, measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps,
                                    advance, stream},
                                   obj_start, obj_goal, is_holding, start_holding, max_turn_steps, stop_turn_steps, min_abs_lin_speed,
                                   allow_sliding);
}

extern "C" int hab_nav2d_rearr_step_geo(void* state, void* geo, const float* dirs, const float* ray, const float* col_cos,
                                        const float* tanv, const int64_t* actions, const uint8_t* mask, uint8_t* head_rgb,
                                        float* head_depth, float* obj_start, float* obj_goal, float* is_holding, float* reward,
                                        uint8_t* not_done, float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H, int W,
                                        int num_obstacles, int num_headings, int max_episode_steps, int start_holding, int advance,
                                        hipStream_t stream) {
    return rearr_step<false, true>({state, geo, dirs, ray, col_cos, tanv, actions, mask, head_rgb, head_depth, nullptr, nullptr, reward,
                                    not_done, measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps,
                                    advance, stream},
                                   obj_start, obj_goal, is_holding, start_holding, 0, 0, 0.0f, 0);
}

extern "C" int hab_nav2d_rearr_vel_step_geo(void* state, void* geo, const float* dirs, const float* ray, const float* col_cos,
                                            const float* tanv, const float* actions, const uint8_t* mask, uint8_t* head_rgb,
                                            float* head_depth, float* obj_start, float* obj_goal, float* is_holding, float* reward,
                                            uint8_t* not_done, float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H,
                                            int W, int num_obstacles, int num_headings, int max_episode_steps, int start_holding,
                                            int max_turn_steps, int stop_turn_steps, float min_abs_lin_speed, int allow_sliding,
                                            int advance, hipStream_t stream) {
    return rearr_step<true, true>({state, geo, dirs, ray, col_cos, tanv, actions, mask, head_rgb, head_depth, nullptr, nullptr, reward,
                                   not_done, measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps,
                                   advance, stream},
                                  obj_start, obj_goal, is_holding, start_holding, max_turn_steps, stop_turn_steps, min_abs_lin_speed,
                                  allow_sliding);
}

// The pick-and-place oracle: the checks of hab_nav2d_rearr_geo_build for state, stride, field, N and K, then those of its own
// arguments.
extern "C" int hab_nav2d_rearr_oracle(const void* state, size_t state_stride_bytes, const void* geo, const float* dirs,
                                      const uint8_t* mask, int64_t* actions, float* next_d, int32_t* status, int N, int num_obstacles,
                                      int num_headings, hipStream_t stream) {
    const int rc = check_geo_args(state, state_stride_bytes, geo, N, num_obstacles);
    if (rc != HAB_OK) return rc;
    if (state_stride_bytes < sizeof(Nav2DRearrState)) return HAB_ERR_ARG;
    if (!guide_args_ok(dirs, actions, sizeof(int64_t), next_d, status, num_headings)) return HAB_ERR_ARG;
    nav2d_rearr_oracle_kernel<<<N, 64, 0, stream>>>((const char*)state, state_stride_bytes, (const RearrGeoField*)geo, dirs, mask, actions,
                                                    next_d, status, num_obstacles, num_headings);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

extern "C" int hab_nav2d_social_state_bytes(void) { return (int)sizeof(Nav2DSocialState); }

// Nav2DSocial-v0: the step (one wavefront per env), the fields of the episodes that began (at a reset, of every env the mask selects),
// then the render.
extern "C" int hab_nav2d_social_step(void* state, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                     const float* actions, const uint8_t* mask, uint8_t* head_rgb, float* head_depth, float* person_sensor,
                                     float* person_visible, float* reward, uint8_t* not_done, float* measure_sums, uint32_t seed,
                                     uint32_t env_offset, int N, int H, int W, int num_obstacles, int num_headings, int max_episode_steps,
                                     int max_turn_steps, int stop_turn_steps, float min_abs_lin_speed, int allow_sliding, float person_speed,
                                     int person_always_visible, int advance, hipStream_t stream) {
    const StepArgs a{state, nullptr, dirs, ray, col_cos, tanv, actions, mask, head_rgb, head_depth, nullptr, nullptr, reward, not_done,
                     measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream};
    const int rc = check_step_args(a, false);
    if (rc != HAB_OK) return rc;
    if (((uintptr_t)state & 3) || ((uintptr_t)actions & 3)) return HAB_ERR_ARG;  // a row of two floats is read as two scalars
    if (!vel_args_ok(max_turn_steps, stop_turn_steps, num_headings)) return HAB_ERR_ARG;
    if (!(person_speed > 0.0f && person_speed <= 0.25f)) return HAB_ERR_ARG;
    if (person_always_visible != 0 && person_always_visible != 1) return HAB_ERR_ARG;
    nav2d_social_step_kernel<<<N, 64, 0, stream>>>((Nav2DSocialState*)state, dirs, actions, mask, person_sensor, person_visible, reward,
                                                   not_done, measure_sums, seed, env_offset, N, num_obstacles, num_headings,
                                                   max_episode_steps, max_turn_steps, stop_turn_steps, min_abs_lin_speed, allow_sliding,
                                                   person_speed, person_always_visible, advance);
    HAB_LAUNCH_CHECK();
    nav2d_social_build_kernel<<<N, 64, 0, stream>>>((Nav2DSocialState*)state, mask, advance ? 1 : 0, num_obstacles);
    HAB_LAUNCH_CHECK();
    return launch_render<Render::SOCIAL>(a, 0);
}

// Nav2DExplore-v0: the step of one workgroup per env over the coverage layer, then the render without a marker.
extern "C" int hab_nav2d_explore_state_bytes(void) { return (int)sizeof(Nav2DExploreState); }

extern "C" int hab_nav2d_explore_step(void* state, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                      const int64_t* actions, const uint8_t* mask, uint8_t* rgb, float* depth, float* gps, float* compass,
                                      const float* compass_table, uint8_t* coverage, float* reward, uint8_t* not_done, float* measure_sums,
                                      uint32_t seed, uint32_t env_offset, int N, int H, int W, int num_obstacles, int num_headings,
                                      int max_episode_steps, int G, float visibility_dist, float rc, int advance, hipStream_t stream) {
    const StepArgs a{state, nullptr, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, nullptr, nullptr, reward, not_done, measure_sums,
                     seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream};
    const int code = check_step_args(a, false, sizeof(Nav2DExploreState));
    if (code != HAB_OK) return code;
    if (((uintptr_t)state & 3) || !coverage || (compass && !compass_table)) return HAB_ERR_ARG;
    if (G < HAB_NAV2D_EXPLORE_MIN_RESOLUTION || G > HAB_NAV2D_EXPLORE_MAX_RESOLUTION) return HAB_ERR_ARG;
    if (!(visibility_dist > 0.f) || !(visibility_dist <= 3.0e38f) || !(rc >= 0.f) || !(rc <= 3.0e38f)) return HAB_ERR_ARG;
    const float cell = ARENA / (float)G;
    const int vec = (G * G) % 4 == 0 && !((uintptr_t)coverage & 3);
    nav2d_explore_step_kernel<<<N, EXPLORE_THREADS, 0, stream>>>((Nav2DExploreState*)state, dirs, compass_table, actions, mask, gps, compass,
                                                                 coverage, reward, not_done, measure_sums, seed, env_offset, N, num_obstacles,
                                                                 num_headings, max_episode_steps, G, cell, visibility_dist,
                                                                 visibility_dist * visibility_dist, rc, advance, vec);
    HAB_LAUNCH_CHECK();
    return launch_render<Render::EXPLORE>(a, 0);
}

// Nav2DImageNav-v0, its two entries like Nav2D-v0's: the step, for a `_geo` entry the fields of the episodes that began, then both
// views in one launch of the render.
extern "C" int hab_nav2d_imagenav_state_bytes(void) { return (int)sizeof(Nav2DImageNavState); }

template <bool GEO>
static int imagenav_step(const StepArgs& a, float* gps, float* compass, const float* compass_table, float success_distance) {
    const int rc = check_step_args(a, GEO, sizeof(Nav2DImageNavState));
    if (rc != HAB_OK) return rc;
    if (((uintptr_t)a.state & 3) || (compass && !compass_table)) return HAB_ERR_ARG;
    if (!(success_distance > 0.f) || !(success_distance <= 3.0e38f)) return HAB_ERR_ARG;
    nav2d_imagenav_step_kernel<GEO><<<cdiv(a.N, 64), 64, 0, a.stream>>>((Nav2DImageNavState*)a.state, a.dirs, compass_table,
                                                                         (const int64_t*)a.actions, a.mask, gps, compass, a.reward, a.not_done,
                                                                         a.measure_sums, a.seed, a.env_offset, a.N, a.num_obstacles,
                                                                         a.num_headings, a.max_episode_steps, success_distance, a.advance,
                                                                         GEO ? (GeoField*)a.geo : nullptr);
    HAB_LAUNCH_CHECK();
    if (GEO) {
        nav2d_geo_build_kernel<<<a.N, 64, 0, a.stream>>>((char*)a.state, sizeof(Nav2DImageNavState), (GeoField*)a.geo, a.mask,
                                                         a.advance ? 1 : 0, a.num_obstacles);
        HAB_LAUNCH_CHECK();
    }
    return launch_render<Render::IMAGENAV>(a, 0);
}

extern "C" int hab_nav2d_imagenav_step(void* state, const float* dirs, const float* ray, const float* col_cos, const float* tanv,
                                       const int64_t* actions, const uint8_t* mask, uint8_t* rgb, float* depth, uint8_t* goal_rgb,
                                       float* gps, float* compass, const float* compass_table, float* reward, uint8_t* not_done,
                                       float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H, int W, int num_obstacles,
                                       int num_headings, int max_episode_steps, float success_distance, int advance, hipStream_t stream) {
    return imagenav_step<false>({state, nullptr, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, nullptr, nullptr, reward, not_done,
                                 measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream,
                                 goal_rgb},
                                gps, compass, compass_table, success_distance);
}

extern "C" int hab_nav2d_imagenav_step_geo(void* state, void* geo, const float* dirs, const float* ray, const float* col_cos,
                                           const float* tanv, const int64_t* actions, const uint8_t* mask, uint8_t* rgb, float* depth,
                                           uint8_t* goal_rgb, float* gps, float* compass, const float* compass_table, float* reward,
                                           uint8_t* not_done, float* measure_sums, uint32_t seed, uint32_t env_offset, int N, int H, int W,
                                           int num_obstacles, int num_headings, int max_episode_steps, float success_distance, int advance,
                                           hipStream_t stream) {
    return imagenav_step<true>({state, geo, dirs, ray, col_cos, tanv, actions, mask, rgb, depth, nullptr, nullptr, reward, not_done,
                                measure_sums, seed, env_offset, N, H, W, num_obstacles, num_headings, max_episode_steps, advance, stream,
                                goal_rgb},
                               gps, compass, compass_table, success_distance);
}
