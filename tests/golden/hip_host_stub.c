// host stand-in for the HIP runtime calls libsignerf_hip.so makes: device memory is host memory, kernels do nothing,
// and the 12-byte device-to-host copy of the table abs-max scan returns the values set with stub_set_absmax
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
typedef struct { uint32_t x, y, z; } dim3_t;
static uint32_t g_absmax[3];
static dim3_t g_grid, g_block; static size_t g_shmem; static void* g_stream;
void stub_set_absmax(const uint32_t* bits) { memcpy(g_absmax, bits, 12); }
int hipMalloc(void** p, size_t n) { *p = calloc(n ? n : 1, 1); return *p ? 0 : 2; }
int hipMallocAsync(void** p, size_t n, void* s) { (void)s; return hipMalloc(p, n); }
int hipFree(void* p) { free(p); return 0; }
int hipFreeAsync(void* p, void* s) { (void)s; free(p); return 0; }
int hipMemcpyAsync(void* d, const void* s, size_t n, int kind, void* st) {
    (void)st;
    if (kind == 2 && n == 12) memcpy(d, g_absmax, 12); else memcpy(d, s, n);
    return 0;
}
int hipMemsetAsync(void* d, int v, size_t n, void* st) { (void)st; memset(d, v, n); return 0; }
int hipMemsetD32Async(void* d, int v, size_t n, void* st) { (void)st; for (size_t i = 0; i < n; ++i) ((int*)d)[i] = v; return 0; }
int hipStreamSynchronize(void* s) { (void)s; return 0; }
int hipStreamWaitEvent(void* s, void* e, unsigned f) { (void)s; (void)e; (void)f; return 0; }
int hipEventCreateWithFlags(void** e, unsigned f) { (void)f; *e = malloc(8); return 0; }
int hipEventDestroy(void* e) { free(e); return 0; }
int hipEventRecord(void* e, void* s) { (void)e; (void)s; return 0; }
int hipEventSynchronize(void* e) { (void)e; return 0; }
int hipGetDevice(int* d) { *d = 0; return 0; }
int hipDeviceGetAttribute(int* v, int a, int d) { (void)a; (void)d; *v = 256; return 0; }
const char* hipGetErrorString(int e) { (void)e; return "stub"; }
int hipGetLastError(void) { return 0; }
int hipLaunchKernel(const void* f, dim3_t g, dim3_t b, void** a, size_t sh, void* st) { (void)f; (void)g; (void)b; (void)a; (void)sh; (void)st; return 0; }
int __hipPushCallConfiguration(dim3_t g, dim3_t b, size_t sh, void* st) { g_grid = g; g_block = b; g_shmem = sh; g_stream = st; return 0; }
int __hipPopCallConfiguration(dim3_t* g, dim3_t* b, size_t* sh, void** st) { *g = g_grid; *b = g_block; *sh = g_shmem; *st = g_stream; return 0; }
static void* g_fat;
void** __hipRegisterFatBinary(const void* d) { (void)d; return &g_fat; }
void __hipRegisterFunction(void** m, const void* hf, char* df, const char* dn, unsigned tl, void* a, void* b, void* c, void* d, int* w) {
    (void)m; (void)hf; (void)df; (void)dn; (void)tl; (void)a; (void)b; (void)c; (void)d; (void)w; }
void __hipUnregisterFatBinary(void** m) { (void)m; }
