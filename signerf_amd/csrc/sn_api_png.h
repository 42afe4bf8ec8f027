// sn_api_png.h (part of sn_api.hip) -- include/signerf_hip_png.h: a device uint8 image to the bytes of its .png file
#pragma once

extern "C" {

int sn_png_abi_version(void) { return SN_PNG_ABI_VERSION; }
size_t sn_png_segment_bytes(void) { return SN_PNG_SEGMENT_BYTES; }
size_t sn_png_max_file_bytes(int32_t h, int32_t w, int32_t c) {
    return sn_png_shape_ok(h, w, c) ? (size_t)sn_png_file_bound((uint32_t)h, (uint32_t)w, (uint32_t)c) : 0;
}
size_t sn_png_workspace_bytes(int32_t h, int32_t w, int32_t c) {
    return sn_png_shape_ok(h, w, c) ? (size_t)sn_png_workspace_size((uint32_t)h, (uint32_t)w, (uint32_t)c) : 0;
}

int sn_png_encode(const uint8_t* image, int32_t h, int32_t w, int32_t c, void* workspace, size_t workspace_bytes, uint8_t* file,
                  size_t file_capacity, uint64_t* file_bytes, SnStream stream) {
    const std::string who = "sn_png_encode";
    if (!image || !workspace || !file || !file_bytes) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (image, workspace, file, file_bytes)");
    if (c != 1 && c != 3) return fail(nullptr, SN_ERR_INVALID, who + ": c must be 1 (greyscale) or 3 (RGB)");
    if (!sn_png_shape_ok(h, w, c)) return fail(nullptr, SN_ERR_INVALID, who + ": h and w must lie in 1..8192");
    if (workspace_bytes < sn_png_workspace_bytes(h, w, c) || ((uintptr_t)workspace & 15u))
        return fail(nullptr, SN_ERR_INVALID, who + ": workspace below sn_png_workspace_bytes, or not 16-byte aligned");
    if (file_capacity < sn_png_max_file_bytes(h, w, c)) return fail(nullptr, SN_ERR_INVALID, who + ": file_capacity below sn_png_max_file_bytes");
    SnPngParams p;
    memset(&p, 0, sizeof(p));
    p.image = image;
    p.h = (uint32_t)h;
    p.w = (uint32_t)w;
    p.c = (uint32_t)c;
    p.row_bytes = p.w * p.c;
    p.stride = 1 + p.row_bytes;
    p.stream_bytes = (uint32_t)sn_png_stream_bytes(p.h, p.w, p.c);
    p.nseg = sn_png_segment_count(p.stream_bytes);
    uint8_t* ws = (uint8_t*)workspace;   // slots (a multiple of 16 bytes each), the offsets, then the 4 uint32 arrays
    p.slots = ws;
    ws += (size_t)p.nseg * SN_PNG_SLOT_STRIDE;
    p.seg_off = (uint64_t*)ws;
    ws += (size_t)p.nseg * 8;
    p.seg_bytes = (uint32_t*)ws;
    p.seg_crc = p.seg_bytes + p.nseg;
    p.seg_adler = p.seg_crc + p.nseg;
    p.file = file;
    p.file_bytes = file_bytes;
    hipStream_t st = (hipStream_t)stream;
    if (c == 1) hipLaunchKernelGGL(sn_png_segment_deflate_kernel<1>, dim3(p.nseg), dim3(64), 0, st, p);
    else hipLaunchKernelGGL(sn_png_segment_deflate_kernel<3>, dim3(p.nseg), dim3(64), 0, st, p);
    hipLaunchKernelGGL(sn_png_finish_file_kernel, dim3(1), dim3(1024), 0, st, p);
    hipLaunchKernelGGL(sn_png_compact_bytes_kernel, dim3(p.nseg), dim3(256), 0, st, p);
    return end_launches(who);
}

}  // extern "C"
