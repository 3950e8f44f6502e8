// C ABI, weights: validate the configuration, pack on the host (pack_host.hpp), upload the arena and fix the pointer table up;
// export / import of a packed arena.
#include "ctx.hpp"
#include "pack_host.hpp"

// arena_src == nullptr: pack from the state_dict entries.  Otherwise (srh_weights_import): the arena LAYOUT depends on cfg alone
// (the same sequence of allocations), so the pointer table is rebuilt without reading a tensor and the packed bytes are copied
// device-to-device from arena_src.
static int pack_impl(srh_ctx* c, const srh_model_cfg* cfg, const srh_named_tensor* tensors, int n, const void* arena_src,
                     size_t arena_src_bytes, srh_weights** out) {
    *out = nullptr;
    const int D = cfg->embed_dim, heads = cfg->num_heads;
    if (D <= 0 || heads <= 0 || D % heads) return fail(c, SRH_ERR_BAD_ARG, "bad embed_dim / num_heads");
    const int hd = D / heads;
    if (hd != 64 && hd != 80) return fail(c, SRH_ERR_UNSUPPORTED, "head_dim must be 64 (MFMA attention kernels) or 80 (ViT-H: generic kernel)");
    // 8 <= S <= 64: the global attention kernels' LDS plan ends at the 64 x 64 window (attention.hip)
    if (cfg->patch_size % 16) return fail(c, SRH_ERR_BAD_ARG, "PATCH_SIZE must be a multiple of 16 from 128 to 1024");
    const int S = cfg->patch_size / 16;
    if (S < 8 || S > 64) return fail(c, SRH_ERR_UNSUPPORTED, "PATCH_SIZE must be a multiple of 16 from 128 to 1024");
    if (cfg->window_size != 14) return fail(c, SRH_ERR_UNSUPPORTED, "window_size must be 14");
    if (D % 128 || (D != 768 && D != 1024 && D != 1280)) return fail(c, SRH_ERR_UNSUPPORTED, "embed_dim must be 768, 1024 or 1280");
    hipSetDevice(c->device);

    srh_weights* w = new srh_weights();
    w->cfg = *cfg; w->S = S; w->D = D; w->heads = heads; w->hd = hd;
    Packer pk;
    pk.layout_only = arena_src != nullptr;
    pk.d2h = [](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    pack_model(pk, w, tensors, n);
    if (!pk.missing.empty()) {
        delete w;
        return fail(c, SRH_ERR_MISSING_WEIGHT, "state_dict entry missing or mis-shaped: " + pk.missing);
    }
    if (arena_src && arena_src_bytes != pk.host.size()) {
        delete w;
        return fail(c, SRH_ERR_BAD_ARG, "srh_weights_import: the packed arena has " + std::to_string(arena_src_bytes) +
                                        " bytes, this configuration packs to " + std::to_string(pk.host.size()));
    }
    hipError_t e = hipMalloc(&w->arena, pk.host.size());
    if (e != hipSuccess) { delete w; return hip_fail(c, e, "hipMalloc(weights)"); }
    w->arena_bytes = pk.host.size();
    e = arena_src ? hipMemcpy(w->arena, arena_src, pk.host.size(), hipMemcpyDeviceToDevice)
                  : hipMemcpy(w->arena, pk.host.data(), pk.host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(w->arena); delete w; return hip_fail(c, e, "hipMemcpy(weights)"); }
    for (auto& f : pk.fix) *f.first = reinterpret_cast<char*>(w->arena) + f.second;
    *out = w;
    return SRH_OK;
}

extern "C" int srh_weights_pack(srh_ctx* c, const srh_model_cfg* cfg, const srh_named_tensor* tensors, int n,
                                srh_weights** out) {
    if (!c || !cfg || !tensors || !out) return fail(c, SRH_ERR_BAD_ARG, "srh_weights_pack: null argument");
    return pack_impl(c, cfg, tensors, n, nullptr, 0, out);
}

extern "C" int srh_weights_export(srh_ctx* c, const srh_weights* w, void* dst, size_t capacity, size_t* bytes) {
    if (!c || !w || !bytes) return fail(c, SRH_ERR_BAD_ARG, "srh_weights_export: null argument");
    *bytes = w->arena_bytes;
    if (!dst) return SRH_OK;
    if (capacity < w->arena_bytes) return fail(c, SRH_ERR_BAD_ARG, "srh_weights_export: destination too small");
    hipSetDevice(c->device);
    const hipError_t e = hipMemcpy(dst, w->arena, w->arena_bytes, hipMemcpyDeviceToDevice);
    return e == hipSuccess ? SRH_OK : hip_fail(c, e, "srh_weights_export");
}

extern "C" int srh_weights_import(srh_ctx* c, const srh_model_cfg* cfg, const void* src, size_t bytes, srh_weights** out) {
    if (!c || !cfg || !src || !out) return fail(c, SRH_ERR_BAD_ARG, "srh_weights_import: null argument");
    return pack_impl(c, cfg, nullptr, 0, src, bytes, out);
}

extern "C" void srh_weights_free(srh_weights* w) {
    if (!w) return;
    if (w->arena) hipFree(w->arena);
    delete w;
}
