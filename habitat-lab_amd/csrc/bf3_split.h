// bf3_split.h -- the exact three-term bf16 split of an fp32 value (the arithmetic every split-bf16 contraction kernel of this
// library is built on: igemm_bf3.h explains why six bf16 products reproduce an fp32 product), and the small pieces those kernels share:
// the order of the six products, the split of eight weights into planes, the LDS transpose read, the item split of a persistent grid.
#pragma once
#include "hab_common.h"

namespace hab {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// (x0, x1) = t1 + t2 + t3 exactly, element-wise, each term a bf16: t1 = rn(x), t2 = rn(x - t1), t3 = x - t1 - t2 (rn = v_cvt_pk_bf16_f32,
// round to nearest even; both residuals are exact in fp32 and the last one has at most 8 significant bits).  Returns the three PACKED
// pairs (low half = element 0).  4.5 VALU instructions per element, packing included.
__device__ __forceinline__ void bf3_split2(float x0, float x1, unsigned& w1, unsigned& w2, unsigned& w3) {
    f32x2 v; v[0] = x0; v[1] = x1;
    w1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    f32x2 r;
    r[0] = v[0] - __uint_as_float(w1 << 16); r[1] = v[1] - __uint_as_float(w1 & 0xffff0000u);
    w2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
    f32x2 q;
    q[0] = r[0] - __uint_as_float(w2 << 16); q[1] = r[1] - __uint_as_float(w2 & 0xffff0000u);
    w3 = __builtin_bit_cast(unsigned, __builtin_convertvector(q, bf16x2));
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));  // one MFMA operand: 8 consecutive k of one row
typedef short v4s __attribute__((ext_vector_type(4)));

// The six partial products of a k-step, smallest weight first: product q multiplies plane BF3_PA[q] of A by plane BF3_PB[q] of B.
// This order is the accuracy contract of the split path (igemm_bf3.h) and is written here only; a kernel keeps its own (unrolled) loop
// over q, its loops over tiles and its own operand order.
constexpr int BF3_PA[6] = {2, 0, 1, 1, 0, 0}, BF3_PB[6] = {0, 2, 1, 0, 1, 0};

// Eight consecutive fp32 values (v0, v1) -> one bf16x8 per plane, each element XORed with sgn2 (0, or 0x80008000: negated).
struct Bf3Planes { bf16x8 p[3]; };
__device__ __forceinline__ Bf3Planes bf3_split8(const f32x4 v0, const f32x4 v1, unsigned sgn2) {
    Bf3Planes o;
    unsigned p[3][4];
    bf3_split2(v0[0], v0[1], p[0][0], p[1][0], p[2][0]);
    bf3_split2(v0[2], v0[3], p[0][1], p[1][1], p[2][1]);
    bf3_split2(v1[0], v1[1], p[0][2], p[1][2], p[2][2]);
    bf3_split2(v1[2], v1[3], p[0][3], p[1][3], p[2][3]);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
        o.p[pl] = __builtin_bit_cast(bf16x8, u32x4{p[pl][0] ^ sgn2, p[pl][1] ^ sgn2, p[pl][2] ^ sgn2, p[pl][3] ^ sgn2});
    return o;
}

// The LDS transpose read (ds_read_b64_tr_b16, semantics pinned on the hardware by tools/ubench/tr_read_probe.hip): lane i of a 16-lane
// group passes the address of ITS 8-byte chunk of a [4 rows][16 elements] block (row i >> 2, chunk i & 3; the rows need not be
// equidistant) and receives element i of the four rows -- the k-contiguous MFMA fragment of a k-strided (pixel-major) image.
__device__ __forceinline__ v4s bf3_tr_read(const unsigned short* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)p);
}
// two transpose reads (k-blocks r = 0, 1 of a lane) make one operand
__device__ __forceinline__ bf16x8 bf3_join(const v4s lo, const v4s hi) {
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// Static split of `items` over a persistent grid (a multiple of 8 workgroups): XCD x = block & 7 takes the x-th eighth of the items
// (consecutive items meet in one L2), its workgroups block >> 3 contiguous pieces of it, in block order.  Block's run: [first, last).
__host__ __device__ inline void xcd_item_run(int items, int block, int grid, int& first, int& last) {
    const int xcd = block & 7, jw = (unsigned)block >> 3, wg_per_xcd = (unsigned)grid >> 3;  // unsigned, as blockIdx.x and gridDim.x are
    const int per_xcd = (items + 7) >> 3, per_wg = (per_xcd + wg_per_xcd - 1) / wg_per_xcd;
    const int xcd_end = min(items, (xcd + 1) * per_xcd);
    first = min(xcd_end, xcd * per_xcd + jw * per_wg);
    last = min(xcd_end, first + per_wg);
}

// The alternating sign schedule of the split-bf16 kernels (igemm_bf3.h), on unless HAB_BF3_NOSIGN is set (development: measures
// its cost).  Read once per process; the launchers run on several inference-worker threads.
inline int bf3_sign_schedule() {
    static const int on = !hab_env_flag("HAB_BF3_NOSIGN");
    return on;
}

}  // namespace hab
