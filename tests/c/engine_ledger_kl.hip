// TEST INFRASTRUCTURE (never part of libvt_hip.so): the recording stand-in of engine_ledger.hip plus the footprints of the KL
// bottleneck's two entry points (include/vt_hip.h, vt_kl_forward / vt_kl_backward), so that a KL handle's schedule can be
// recorded too.  tests/test_kl_cpu.py links it with the product objects vt_engine.o + vt_api.o, whose weak references to the two
// entry points bind here.
#include "engine_ledger.hip"

extern "C" int vt_kl_forward(const float* z, int64_t ldz, int64_t M, int32_t d, int32_t, uint64_t, const uint32_t* ctr, float* mean,
                             float* sample, void* rzp, int64_t ldp, float* noise, float* loss, void* ws, vtStream s) {
    Rec rec("kl_forward", s);
    rec.mat(z, M, 2 * d, ldz, 4, false); rec.r(ctr, 4);
    rec.w(mean, (size_t)M * d * 4); rec.w(sample, (size_t)M * d * 4); rec.w(noise, (size_t)M * d * 4);
    rec.mat(rzp, M, ldp, ldp, 2, true); rec.w(loss, 4);
    rec.r(ws, VT_KL_WORKSPACE_BYTES); rec.w(ws, VT_KL_WORKSPACE_BYTES);
    return VT_OK;
}
extern "C" int vt_kl_backward(const float* g, int64_t ldg, const float* gmean, const float* gkl, const float* z, int64_t ldz, const float* noise,
                              int64_t M, int32_t d, int32_t, float* dz, void* dzp, int64_t ldp, vtStream s) {
    Rec rec("kl_backward", s);
    rec.mat(g, M, d, ldg, 4, false); rec.r(gmean, (size_t)M * d * 4); rec.r(gkl, 4);
    rec.mat(z, M, 2 * d, ldz, 4, false); rec.r(noise, (size_t)M * d * 4);
    rec.w(dz, (size_t)M * 2 * d * 4); rec.mat(dzp, M, ldp, ldp, 2, true);
    return VT_OK;
}
