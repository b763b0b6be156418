// jpezy_capi_resized.hip -- the C-ABI of include/jpezy_hip.h, part 14: a batch of windows, resized.  The two pure host functions of the
// section (the tap tables of one axis, the window and scale for a source rectangle), part 15's (scale and bias of a tensor output from mean
// and std) and the host side of the second stage: descriptors
// and tap tables of a launch of resample_kernel (jpezy_kernels_resized.hip), built in the context's pinned staging and uploaded in one
// copy.  The entry itself, jpezy_decode_windows_resized_dev, shares its driver with jpezy_decode_windows_dev (jpezy_capi_windows.hip).
#include "jpezy_capi_decode.h"
#include "jpezy_resize_taps.h"
#include "jpezy_tensor_layout.h"

#include <map>
#include <tuple>

extern "C" {

// One launch sequence over `jobs`: windows of packed pixels behind d_src (rows src_stride apart) to out_w x out_h pixels behind d_dst (rows
// dst_stride apart).  Asynchronous on s; c->r_pin is the caller's to keep until s has passed the upload.  t0, t1 (both or neither): events
// recorded in front of the upload and behind the last launch.  tensor: the launch is resample_tensor_kernel's, d_dst the tensor's first
// element, ResampleJob::dst_off in elements, dst_stride not read (jpezy_device.h, TensorOut).
// how.filter other than the triangle: the launch is the kernels' two-pass instance, and a file runs the tile when its y table's largest
// tile span fits kResampleTileRows -- decided per file, here; the triangle filter, how.direct and a launch without any such file keep
// the direct instance.
int jpezy_internal_resample(jpezy_ctx* c, const std::vector<ResampleJob>& jobs, const uint8_t* d_src, unsigned src_stride, uint8_t* d_dst,
                            size_t dst_stride, int out_w, int out_h, int bytes, hipStream_t s, const ResampleHow& how, int* tiled, hipEvent_t t0,
                            hipEvent_t t1, const TensorOut* tensor)
{
    if (tiled) *tiled = 0;
    if (jobs.empty()) return JPEZY_OK;
    if (!jpezy_host::resize_filter_known(how.filter)) return set_err(JPEZY_E_BADARG, "resample: unknown filter");
    // tap tables, one per distinct (filter, source size, output size) of either axis: first | count << 16 per output index
    // (count <= in_size <= 65535), then the weights
    struct Tab { unsigned fc, w; int ksize, span; bool fits; };
    std::map<std::tuple<int, int, int>, Tab> tabs;
    std::vector<int> taps;
    auto table = [&](int in_size, int out_size) -> const Tab& {
        const auto key = std::make_tuple(how.filter, in_size, out_size);
        auto it = tabs.find(key);
        if (it != tabs.end()) return it->second;
        const jpezy_host::ResizeTaps t = jpezy_host::resize_taps(how.filter, in_size, out_size);
        // span: of a tile of kResampleTileH output ROWS (read for the y table of a file only)
        const Tab tb = { (unsigned)taps.size(), (unsigned)(taps.size() + (size_t)out_size), t.ksize,
                         jpezy_host::resize_tile_span(t.first.data(), t.count.data(), out_size, kResampleTileH), t.fits };
        for (int i = 0; i < out_size; ++i) taps.push_back((int)((unsigned)t.first[(size_t)i] | (unsigned)t.count[(size_t)i] << 16));
        taps.insert(taps.end(), t.weight.begin(), t.weight.end());
        return tabs.emplace(key, tb).first->second;
    };
    const unsigned long long tiles = (unsigned long long)((out_w + kResampleTileW - 1) / kResampleTileW) * (unsigned long long)((out_h + kResampleTileH - 1) / kResampleTileH);
    std::vector<ResampleDesc> desc(jobs.size());
    unsigned long long total = 0;
    const bool may_tile = how.filter != JPEZY_FILTER_BILINEAR && !how.direct;
    int n_tiled = 0;
    for (size_t k = 0; k < jobs.size(); ++k) {
        const ResampleJob& j = jobs[k];
        const Tab tx = table(j.w, out_w), ty = table(j.h, out_h);      // (copies: the map may grow between the two)
        if (!tx.fits || !ty.fits)
            return set_err(JPEZY_E_UNSUPPORTED, "resample: the weights of " + std::to_string(j.w) + " x " + std::to_string(j.h) + " to " + std::to_string(out_w) +
                                                    " x " + std::to_string(out_h) + " could overflow a 32-bit accumulator");
        if (taps.size() > 0x7FFFFFFFull || total + tiles > 0xFFFFFFFFull)
            return set_err(JPEZY_E_NOSPACE, "resample: the tap tables or the workgroups of one launch do not fit in 32 bits");
        ResampleDesc& d = desc[k];
        std::memset(&d, 0, sizeof d);
        d.src_off = j.src_off; d.dst_off = j.dst_off;
        d.xfc = tx.fc; d.xw = tx.w; d.yfc = ty.fc; d.yw = ty.w;
        d.w = j.w; d.h = j.h; d.kx = tx.ksize; d.ky = ty.ksize;
        d.mirror = j.mirror ? 1 : 0;
        d.tiled = may_tile && ty.span <= kResampleTileRows ? 1u : 0u;
        n_tiled += (int)d.tiled;
        d.wg0 = (unsigned)total;
        total += tiles;
    }
    const size_t desc_bytes = desc.size() * sizeof(ResampleDesc), bytes_all = desc_bytes + taps.size() * sizeof(int);
    if (int rc = c->r_pin.reserve(bytes_all, bytes_all + (bytes_all >> 2))) return rc;
    if (int rc = c->r_tab.reserve(bytes_all)) return rc;
    std::memcpy(c->r_pin.p, desc.data(), desc_bytes);
    std::memcpy(c->r_pin.p + desc_bytes, taps.data(), taps.size() * sizeof(int));
    if (t0) HIP_TRY(hipEventRecord(t0, s));
    HIP_TRY(hipMemcpyAsync(c->r_tab.p, c->r_pin.p, bytes_all, hipMemcpyHostToDevice, s));
    ResampleParams p;
    std::memset(&p, 0, sizeof p);
    p.src = d_src;
    p.desc = (const ResampleDesc*)c->r_tab.p;
    p.taps = (const int*)((const uint8_t*)c->r_tab.p + desc_bytes);
    p.dst = d_dst;
    p.n_desc = (unsigned)desc.size();
    p.src_stride = src_stride; p.dst_stride = (unsigned)dst_stride;
    p.out_w = out_w; p.out_h = out_h;
    p.pix_bytes = bytes;
    HIP_TRY(tensor ? launch_resample_tensor(p, *tensor, total, s, n_tiled > 0) : launch_resample(p, total, s, n_tiled > 0));
    if (t1) HIP_TRY(hipEventRecord(t1, s));
    if (tiled) *tiled = n_tiled;
    return JPEZY_OK;
}

int jpezy_resize_taps_filter(int filter, int in_size, int out_size, int* ksize, int* first, int* count, int32_t* weight, size_t weight_cap)
try {
    const char* who = "resize_taps";
    static_assert(JPEZY_FILTER_BILINEAR == jpezy_host::kFilterBilinear && JPEZY_FILTER_BOX == jpezy_host::kFilterBox &&
                  JPEZY_FILTER_BICUBIC == jpezy_host::kFilterBicubic && JPEZY_FILTER_LANCZOS == jpezy_host::kFilterLanczos, "jpezy_resize_taps.h");
    if (!jpezy_host::resize_filter_known(filter)) return set_err(JPEZY_E_BADARG, std::string(who) + ": filter must be one of JPEZY_FILTER_*");
    if (in_size < 1 || in_size > 65535 || out_size < 1 || out_size > 65535)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": in_size and out_size must be in 1..65535");
    if (!ksize) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    *ksize = jpezy_host::resize_ksize(filter, in_size, out_size);
    if (!first && !count && !weight) return JPEZY_OK;
    if (!first || !count || !weight) return set_err(JPEZY_E_BADARG, std::string(who) + ": first, count and weight are given together or not at all");
    if (weight_cap < (size_t)out_size * (size_t)*ksize)
        return set_err(JPEZY_E_NOSPACE, std::string(who) + ": weight_cap is below out_size * ksize = " + std::to_string((size_t)out_size * (size_t)*ksize));
    if (!jpezy_host::resize_taps_into(filter, in_size, out_size, *ksize, first, count, weight))
        return set_err(JPEZY_E_UNSUPPORTED, std::string(who) + ": the weights of an output index could overflow a 32-bit accumulator");
    return JPEZY_OK;
}
JPEZY_CATCH

int jpezy_resize_taps(int in_size, int out_size, int* ksize, int* first, int* count, int32_t* weight, size_t weight_cap)
{
    return jpezy_resize_taps_filter(JPEZY_FILTER_BILINEAR, in_size, out_size, ksize, first, count, weight, weight_cap);
}

int jpezy_resize_pick_window(int W, int H, const jpezy_rect* src, int out_w, int out_h, jpezy_window* win)
{
    const char* who = "resize_pick_window";
    if (!src || !win) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (W <= 0 || H <= 0) return set_err(JPEZY_E_BADARG, std::string(who) + ": width and height must be positive");
    if (out_w < 1 || out_h < 1 || out_w > 65535 || out_h > 65535) return set_err(JPEZY_E_BADARG, std::string(who) + ": out_w and out_h must be in 1..65535");
    if (int rc = region_inside(who, W, H, 1, src)) return rc;
    int s = 1;
    for (int t = 8; t > 1; t >>= 1)
        if (src->w / t >= out_w && src->h / t >= out_h) { s = t; break; }
    *win = { { src->x / s, src->y / s, std::max(1, src->w / s), std::max(1, src->h / s) }, s };
    return JPEZY_OK;
}

int jpezy_tensor_normalization(int C, const double* mean, const double* std_, float* scale, float* bias)
{
    const char* who = "tensor_normalization";
    if (C != 1 && C != 3) return set_err(JPEZY_E_BADARG, std::string(who) + ": C must be 3 or 1");
    if (!mean || !std_ || !scale || !bias) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (!jpezy_host::tensor_normalization(C, mean, std_, scale, bias))
        return set_err(JPEZY_E_BADARG, std::string(who) + ": every std must be finite and not zero, every mean finite");
    return JPEZY_OK;
}

}  // extern "C"
