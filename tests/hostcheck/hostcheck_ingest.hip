// TEST INFRASTRUCTURE ONLY -- CPU executor for the per-pixel arithmetic of the table-driven observation ingest.
//
// ingest_table_kernel (csrc/resnet_ops.hip) computes every output pixel with `ingest_table_pixel` (csrc/resnet_ops.h), which is
// `__host__ __device__`: this file runs the *same function* in a plain loop on host memory, so that the CPU test-suite pins the scaling,
// the order of the four taps, the unpacking of the 16-bit / 8-byte units and the channel offsets bit for bit against F.avg_pool2d
// (tests/test_fused_sensors_host.py) without a GPU.  Built into tests/hostcheck/libhab_hostcheck_ingest.so; never loaded by the product.
#include "../../habitat-lab_amd/csrc/resnet_ops.h"

using namespace hab;

// y[f][ho][wo][0 .. cpad) for B frames read through rows[] (nullable); returns 0 or a negative HAB_ERR_*.  vec_used (nullable): how many
// sensors take the paired-tap loads.
extern "C" int hc_ingest_table(const void* const* sensors, const int* dtypes, const int* channels, const float* scales, int n,
                               const int* rows, float* y, int B, int H, int W, int cpad, int* vec_used) {
    if (!sensors || !dtypes || !channels || !scales || !y || n <= 0 || n > INGEST_MAX_SENSORS || B <= 0 || H < 2 || W < 2) return HAB_ERR_ARG;
    IngestTable t{};
    t.n = n;
    for (int i = 0; i < n; ++i) {
        if (channels[i] <= 0 || channels[i] > 8 || dtypes[i] < 0 || dtypes[i] > 2) return HAB_ERR_ARG;
        t.src[i] = sensors[i]; t.dtype[i] = (signed char)dtypes[i]; t.ch[i] = (signed char)channels[i]; t.scale[i] = scales[i];
    }
    int creal = 0;
    const int rc = ingest_table_finish(t, W, cpad, &creal);
    if (rc != HAB_OK) return rc;
    if (vec_used) { *vec_used = 0; for (int i = 0; i < n; ++i) *vec_used += t.vec[i]; }
    const int Ho = H / 2, Wo = W / 2;
    for (int f = 0; f < B; ++f)
        for (int ho = 0; ho < Ho; ++ho)
            for (int wo = 0; wo < Wo; ++wo) {
                const size_t srow = rows ? rows[f] : f;
                const size_t px = (srow * H + 2 * ho) * W + 2 * wo;
                float out[8];
                ingest_table_pixel(t, px, W, out);
                float* o = y + (((size_t)f * Ho + ho) * Wo + wo) * cpad;
                for (int c = 0; c < cpad; ++c) o[c] = out[c];
            }
    return HAB_OK;
}
