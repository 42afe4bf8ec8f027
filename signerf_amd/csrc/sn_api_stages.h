// sn_api_stages.h (part of sn_api.hip) -- the single stages of include/signerf_hip.h that take no handle: sample positions, compositing,
// PDF sampling, the uint8 conversion, the bilinear resize and the clock probe
#pragma once

extern "C" {

int sn_debug_sample_positions(const float* origins, const float* directions, const float* starts, const float* ends, int64_t n,
                              float* q_strict, float* q_exact, float* q_fast, SnStream stream) {
    if (!origins || !directions || !starts || !ends || n < 0) return fail(nullptr, SN_ERR_INVALID, "sn_debug_sample_positions: bad argument");
    if (n == 0) return SN_OK;
    hipLaunchKernelGGL(sn_debug_sample_positions_kernel, blocks_for(n), dim3(256), 0, (hipStream_t)stream, origins, directions, starts, ends, n,
                       q_strict, q_exact, q_fast);
    return end_launches("sn_debug_sample_positions");
}

int sn_composite(const float* euclid_bins, const float* density, const float* rgb_samples, int64_t n_rays, int32_t n_samples,
                 float* weights, float* rgb, float* depth, int32_t* median_index, float* accumulation, float* expected_depth,
                 SnStream stream) {
    if (!euclid_bins || !density || !rgb_samples || n_rays < 0 || n_samples < 1)
        return fail(nullptr, SN_ERR_INVALID, "sn_composite: bad argument");
    if (n_rays == 0) return SN_OK;
    hipStream_t st = (hipStream_t)stream;
    SnCompositeStageParams p;
    memset(&p, 0, sizeof(p));
    p.bins = euclid_bins;
    p.density = density;
    p.rgb_s = rgb_samples;
    p.n_rays = n_rays;
    p.n_samples = n_samples;
    p.weights = weights;
    p.rgb = rgb;
    p.depth = depth;
    p.median_index = median_index;
    p.acc = accumulation;
    uint32_t* mm = nullptr;
    if (expected_depth) {
        // expected_depth doubles as the raw buffer; min/max live in a small stream-ordered allocation
        if (hipMallocAsync((void**)&mm, 8, st) != hipSuccess) return fail(nullptr, SN_ERR_HIP, "sn_composite: hipMallocAsync failed");
        if (hipMemsetAsync(mm, 0xff, 4, st) != hipSuccess || hipMemsetAsync(mm + 1, 0x00, 4, st) != hipSuccess)
            return fail(nullptr, SN_ERR_HIP, "sn_composite: memset failed");
        p.exp_raw = expected_depth;
        p.minmax = mm;
    }
    hipLaunchKernelGGL(sn_composite_kernel, blocks_for(n_rays, 128), dim3(128), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && expected_depth) {
        hipLaunchKernelGGL(sn_clip_expected_kernel, blocks_for(n_rays), dim3(256), 0, st, expected_depth, mm, n_rays, 0x7fffffff, 1, expected_depth);
        e = hipGetLastError();
        (void)hipFreeAsync(mm, st);
    }
    if (e != hipSuccess) return fail(nullptr, SN_ERR_HIP, std::string("sn_composite launch: ") + hipGetErrorString(e));
    return SN_OK;
}

int sn_pdf_sample(const float* spacing_bins, const float* weights, int64_t n_rays, int32_t n_in, int32_t n_out, const float* u,
                  float histogram_padding, float* new_bins, int32_t* inds, SnStream stream) {
    if (!spacing_bins || !weights || !u || !new_bins || n_rays < 0 || n_in < 1 || n_in > SN_PROP_MAX_SAMPLES || n_out < 1 ||
        n_out > SN_PROP_MAX_SAMPLES)
        return fail(nullptr, SN_ERR_INVALID, "sn_pdf_sample: bad argument");
    if (n_rays == 0) return SN_OK;
    SnPdfStageParams p;
    memset(&p, 0, sizeof(p));
    p.sbins = spacing_bins;
    p.weights = weights;
    p.n_rays = n_rays;
    p.n_in = n_in;
    p.n_out = n_out;
    p.u = u;
    p.hist_pad = histogram_padding;
    p.new_bins = new_bins;
    p.inds = inds;
    hipLaunchKernelGGL(sn_pdf_stage_kernel, blocks_for(n_rays, 64), dim3(64), 0, (hipStream_t)stream, p);
    return end_launches("sn_pdf_sample");
}

int sn_tensor_to_uint8(const float* in, int64_t n, uint8_t* out, SnStream stream) {
    if (!in || !out || n < 0) return fail(nullptr, SN_ERR_INVALID, "sn_tensor_to_uint8: bad argument");
    if (n == 0) return SN_OK;
    hipLaunchKernelGGL(sn_tensor_to_uint8_kernel, blocks_for(n), dim3(256), 0, (hipStream_t)stream, in, n, out);
    return end_launches("sn_tensor_to_uint8");
}

int sn_resize_bilinear(const void* src, int32_t src_u8, int32_t src_h, int32_t src_w, int64_t src_row_stride, int32_t channels, float* dst,
                       int32_t dst_h, int32_t dst_w, int64_t dst_row_stride, int32_t threshold, SnStream stream) {
    if (!src || !dst || src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || channels < 1 ||
        src_row_stride < (int64_t)src_w * channels || dst_row_stride < (int64_t)dst_w * channels)
        return fail(nullptr, SN_ERR_INVALID, "sn_resize_bilinear: bad argument");
    SnResizeParams p;
    memset(&p, 0, sizeof(p));
    p.src = src;
    p.dst = dst;
    p.src_u8 = src_u8 != 0;
    p.src_h = src_h;
    p.src_w = src_w;
    p.dst_h = dst_h;
    p.dst_w = dst_w;
    p.channels = channels;
    p.src_row_stride = src_row_stride;
    p.dst_row_stride = dst_row_stride;
    p.threshold = threshold != 0;
    hipLaunchKernelGGL(sn_resize_bilinear_kernel, blocks_for((int64_t)dst_h * dst_w * channels), dim3(256), 0, (hipStream_t)stream, p);
    return end_launches("sn_resize_bilinear");
}

// one wave per workgroup: shader-clock cycles (s_memtime) elapsed while the constant-rate wall clock (s_memrealtime) advances by `ticks`.
// EIGHT workgroups, one per XCD (the dispatcher places block b on XCD b % 8): the XCDs of one part do not run at one clock under load
// (measured r04, profiles/r04_power_data_activity.txt: 1.84 .. 1.99 GHz side by side, persistently), so a single wave reports whichever die it
// lands on; the sums over the eight give the mean.
__global__ void sn_clock_probe_kernel(unsigned long long* out, unsigned long long ticks) {
    const unsigned long long r0 = wall_clock64();
    const unsigned long long c0 = __builtin_readcyclecounter();
    while (wall_clock64() - r0 < ticks) __builtin_amdgcn_s_sleep(32);
    const unsigned long long c1 = __builtin_readcyclecounter();
    const unsigned long long r1 = wall_clock64();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], c1 - c0);
        atomicAdd(&out[1], r1 - r0);
    }
}

int sn_clock_probe(uint64_t* out, double seconds, SnStream stream) {
    if (!out || !(seconds > 0.0) || seconds > 1.0) return fail(nullptr, SN_ERR_INVALID, "sn_clock_probe: bad argument (0 < seconds <= 1)");
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
        return fail(nullptr, SN_ERR_HIP, "sn_clock_probe: cannot read the wall-clock rate of the device");
    const unsigned long long rate = (unsigned long long)khz * 1000ull;
    const unsigned long long ticks = (unsigned long long)(seconds * (double)rate);
    hipError_t e = hipMemsetAsync(out, 0, 16, (hipStream_t)stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sn_clock_probe_kernel, dim3(8), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)out, ticks);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out + 2, &rate, 8, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, SN_ERR_HIP, std::string("sn_clock_probe: ") + hipGetErrorString(e));
    return SN_OK;
}

}  // extern "C"
