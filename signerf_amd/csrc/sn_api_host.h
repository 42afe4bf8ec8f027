// sn_api_host.h -- what the host code of every entry point shares: the error text, the versioned-struct copy, the launch epilogue and the
// block count.  Included by sn_api.hip (one translation unit) before the files that hold the entry points without a handle (sn_api_*.h).
#pragma once

namespace {

// the text goes to the handle, or without one to the calling thread's sn_last_error(NULL) text (sn_api.hip)
int fail(SnHandle h, int code, const std::string& msg);

#define SN_HIP(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) return fail(h, SN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// include/signerf_hip.h "ABI evolution": the caller's struct begins with the sizeof ITS header gives it.  Exactly that many bytes are
// copied into the library's own (zeroed) struct: fields the caller does not know keep their zero defaults, nothing behind the caller's
// struct is read.  min_size = the struct's size in the first versioned header (r06).
template <typename T>
int adopt_struct(SnHandle h, const T* in, size_t min_size, T& out, const char* what) {
    memset((void*)&out, 0, sizeof(T));
    uint32_t sz = 0;
    memcpy(&sz, (const void*)in, sizeof(sz));
    if (sz < min_size || sz > sizeof(T))
        return fail(h, SN_ERR_INVALID, std::string(what) + ".struct_size = " + std::to_string(sz) + ": this library (SN_ABI_VERSION " + std::to_string(SN_ABI_VERSION) +
                                           ") knows sizes " + std::to_string(min_size) + " .. " + std::to_string(sizeof(T)) +
                                           (sz == 0 ? " -- struct_size was not set (set it to sizeof of the struct in your header)"
                                                    : sz > sizeof(T) ? " -- the caller was built against a newer header than the library" : ""));
    memcpy((void*)&out, (const void*)in, sz);
    out.struct_size = (uint32_t)sizeof(T);
    return SN_OK;
}

void clear_stamp(const void* ws);  // (sn_api.hip) SnRenderOpts.reuse_final_bins: whoever else is handed a workspace clears its stamp

// after the last launch of the entry point `who`
int end_launches(const std::string& who) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, SN_ERR_HIP, who + " launch: " + hipGetErrorString(e));
    return SN_OK;
}

dim3 blocks_for(int64_t n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }  // blocks of `block` lanes covering n

}  // namespace
