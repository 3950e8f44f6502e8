// C ABI of libsamroad_hip.so (declared in include/samroad_hip.h), context part: ABI version and build id, context lifetime, the
// non-finite sentinel and the profiler.  The other parts: api_weights.hip, api_model.hip, api_scene.hip, api_ops.hip (test-only entries).
#include <cstdio>
#include <cstring>

#include "ctx.hpp"

// ---- the profiler's bookkeeping behind run() (ctx.hpp) --------------------------------------------
int cls_id(srh_ctx* c, const char* name) {
    for (size_t i = 0; i < c->cls_names.size(); ++i)
        if (c->cls_names[i] == name) return (int)i;
    c->cls_names.push_back(name);
    return (int)c->cls_names.size() - 1;
}
hipEvent_t next_event(srh_ctx* c) {
    if (c->ev_used == c->ev_pool.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        c->ev_pool.push_back(e);
    }
    return c->ev_pool[c->ev_used++];
}

// ---- C ABI: lifetime -----------------------------------------------------------------------------
extern "C" int srh_abi_version(void) { return SRH_ABI_VERSION; }

#ifndef SRH_BUILD_ID_HEX
#define SRH_BUILD_ID_HEX "unstamped-build!"
#endif
// sha256 of the sources this library was compiled from (sam_road_amd/build.py source_id); the marker is also what build.py
// greps the file for
static const char kBuildId[] = "SRH_BUILD_ID=" SRH_BUILD_ID_HEX;
extern "C" const char* srh_build_id(void) { return kBuildId + 13; }

extern "C" int srh_ctx_create(int device, srh_ctx** out) {
    if (!out) return SRH_ERR_BAD_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return SRH_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return SRH_ERR_HIP;
    srh_ctx* c = new srh_ctx();
    c->device = device;
    void* h = nullptr; void* d = nullptr;
    if (hipHostMalloc(&h, NF_SLOTS * sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        if (h) hipHostFree(h);
        delete c;
        return SRH_ERR_HIP;
    }
    memset(h, 0, NF_SLOTS * sizeof(unsigned));
    c->nf_host = (unsigned*)h; c->nf_dev = (unsigned*)d;
    *out = c;
    return SRH_OK;
}

extern "C" void srh_ctx_destroy(srh_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->lane_stream) hipStreamDestroy(c->lane_stream);   // every call joined it to its caller's stream; what is queued still completes
    if (c->lane_fork) hipEventDestroy(c->lane_fork);
    if (c->lane_join) hipEventDestroy(c->lane_join);
    if (c->clean_done) hipEventDestroy(c->clean_done);
    for (DevBuf* b : c->bufs) b->release();
    c->ztab.release();
    if (c->nf_host) hipHostFree(c->nf_host);
    for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
    delete c;
}

extern "C" size_t srh_ctx_device_bytes(const srh_ctx* c) {
    if (!c) return 0;
    size_t n = c->ztab.device_bytes();
    for (const DevBuf* b : c->bufs) n += b->cap;
    return n;
}

extern "C" int srh_ctx_set_lanes(srh_ctx* c, int mode) {
    if (!c) return SRH_ERR_BAD_ARG;
    if (mode < 0 || mode > 2) return fail(c, SRH_ERR_BAD_ARG, "srh_ctx_set_lanes: mode must be 0 (auto), 1 (one lane) or 2 (two lanes whenever B is even)");
    c->lanes_mode = mode;
    return 0;
}
extern "C" int srh_ctx_last_lanes(const srh_ctx* c) { return c ? c->last_lanes : 0; }

extern "C" const char* srh_last_error(const srh_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

// The sentinel flags as the host sees them NOW (no synchronisation): SRH_ERR_NONFINITE + a message naming the first stage that saw an
// Inf / NaN, flags cleared; 0 if none is set.  The reference's own guards (inferencer.py:206 NaN -> -100, :219 assert 0 <= score <= 1)
// only look at TopoNet's output; an fp16 overflow in the encoder would otherwise come out as silently wrong masks.
int nonfinite_check(srh_ctx* c, const char* who) {
    if (!c->nf_host) return 0;
    int first = -1;
    for (int i = 0; i < NF_SLOTS; ++i)
        if (reinterpret_cast<volatile unsigned*>(c->nf_host)[i]) { if (first < 0) first = i; c->nf_host[i] = 0; }
    if (first < 0) return 0;
    if (first == NF_PAIRS)
        return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": an earlier srh_toponet_ragged call on this context was given a pair that names a row "
                                        "outside its own tile (or outside [0, R)); the scores of that call are invalid");
    std::string where;
    if (first < NF_NECK) where = "encoder block " + std::to_string(first / 2) + (first & 1 ? ", norm2 (the block's attention branch output or its residual stream)"
                                                                                         : ", norm1 (the previous block's MLP output, the patch embedding for block 0, or the residual stream)");
    else if (first < NF_DECODER) where = std::string("neck LayerNorm2d ") + (first == NF_NECK ? "1 (the last block's output)" : "2");
    else where = "map_decoder LayerNorm2d";
    return fail(c, SRH_ERR_NONFINITE, std::string(who) + ": non-finite activations (fp16 overflow?) in an earlier call on this context, first seen by " + where +
                                      "; the outputs of that call are invalid");
}

extern "C" int srh_ctx_check(srh_ctx* c, void* stream, int synchronize) {
    if (!c) return SRH_ERR_BAD_ARG;
    if (synchronize) {
        hipSetDevice(c->device);
        const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(c, e, "srh_ctx_check");
    }
    return nonfinite_check(c, "srh_ctx_check");
}

// ---- profiling ------------------------------------------------------------------------------------------------
extern "C" int srh_profile_enable(srh_ctx* c, int on) {
    if (!c) return SRH_ERR_BAD_ARG;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    c->profiling = on != 0;
    c->prof.clear();
    c->ev_used = 0;
    return 0;
}

// one wave that spins until the 100 MHz constant-rate clock has advanced by `ticks`: a kernel of KNOWN duration
__global__ void srh_spin_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(2);
}

// What an event pair around ONE launch adds beyond the time the kernel's waves run: median over 32 launches of (event-to-event
// time around a kernel whose single wave spins for exactly 50 us) - 50 us, measured on `stream` with the device otherwise idle
// (~3 us on MI355X: dispatch-to-first-wave, last-wave-to-completion and the marker packets).  Informational: rocprofv3 counts
// most of it as kernel duration too — bench.py's raw event times agree with `rocprofv3 --kernel-trace --stats` to ~1 %
// (profiles/r03_event_overhead_check.txt).
extern "C" int srh_profile_overhead(srh_ctx* c, void* stream, double* ms_per_launch) {
    if (!c || !ms_per_launch) return SRH_ERR_BAD_ARG;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int N = 32;
    const unsigned long long ticks = 5000;                      // 50 us at the 100 MHz wall clock
    std::vector<hipEvent_t> ev(2 * N);
    for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) return fail(c, SRH_ERR_HIP, "hipEventCreate failed");
    for (int warm = 0; warm < 2; ++warm)
        for (int i = 0; i < N; ++i) {
            hipEventRecord(ev[2 * i], s);
            hipLaunchKernelGGL(srh_spin_kernel, dim3(1), dim3(64), 0, s, ticks);
            hipEventRecord(ev[2 * i + 1], s);
        }
    hipError_t e = hipStreamSynchronize(s);
    std::vector<float> d(N);
    for (int i = 0; i < N; ++i) hipEventElapsedTime(&d[i], ev[2 * i], ev[2 * i + 1]);
    for (auto& x : ev) hipEventDestroy(x);
    if (e != hipSuccess) return hip_fail(c, e, "srh_profile_overhead");
    std::sort(d.begin(), d.end());
    *ms_per_launch = std::max(0.0, (double)d[N / 2] - 0.050);
    return 0;
}

extern "C" int srh_profile_read(srh_ctx* c, srh_profile_row* rows, int max_rows, int* n_rows) {
    if (!c || !rows || !n_rows) return SRH_ERR_BAD_ARG;
    hipSetDevice(c->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(c, e, "hipDeviceSynchronize");
    std::vector<srh_profile_row> acc(c->cls_names.size());
    for (size_t i = 0; i < acc.size(); ++i) {
        memset(&acc[i], 0, sizeof(srh_profile_row));
        snprintf(acc[i].name, sizeof(acc[i].name), "%s", c->cls_names[i].c_str());
    }
    for (const ProfEntry& pe : c->prof) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, pe.e0, pe.e1);
        acc[pe.cls].launches += 1;
        acc[pe.cls].ms += ms;
        acc[pe.cls].flops += pe.flops;
        acc[pe.cls].bytes += pe.bytes;
    }
    int k = 0;
    for (size_t i = 0; i < acc.size() && k < max_rows; ++i)
        if (acc[i].launches) rows[k++] = acc[i];
    *n_rows = k;
    c->prof.clear();
    c->ev_used = 0;
    return 0;
}
