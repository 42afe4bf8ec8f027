// host stand-in for the HIP runtime calls libsignerf_hip.so makes: device memory is host memory from ONE reserved arena (so "is a device
// pointer" is a range check), kernels do nothing but are logged -- registered name, grid, block, LDS bytes and their arguments, in which
// every aligned 8-byte word that points into the arena is replaced by its offset from the arena's base -- and the 12-byte device-to-host
// copy of the table abs-max scan returns the values set with stub_set_absmax
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
typedef struct { uint32_t x, y, z; } dim3_t;
static uint32_t g_absmax[3];
static dim3_t g_grid, g_block; static size_t g_shmem; static void* g_stream;
void stub_set_absmax(const uint32_t* bits) { memcpy(g_absmax, bits, 12); }

// ---- the arena: bump allocation, a freed block is handed out again to a request of exactly its size; every block starts zeroed --------
#define ARENA_BYTES (1ull << 34)
#define BIG (1u << 20)   // blocks from this size on are page aligned and zeroed by giving their pages back
typedef struct { size_t off, n; int is_free; } block_t;
static char* g_arena; static size_t g_top; static block_t g_blocks[8192]; static int g_nblocks;
static int in_arena(const void* p) { return g_arena && (const char*)p >= g_arena && (const char*)p < g_arena + ARENA_BYTES; }
static void zero(char* p, size_t n) {
    if (n >= BIG && in_arena(p) && ((uintptr_t)p & 4095) == 0) {
        const size_t whole = n & ~(size_t)4095;
        madvise(p, whole, MADV_DONTNEED);   // (private anonymous pages read as zero again)
        memset(p + whole, 0, n - whole);
    } else memset(p, 0, n);
}
int hipMalloc(void** p, size_t n) {
    if (!g_arena) {
        g_arena = (char*)mmap(NULL, ARENA_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (g_arena == (char*)MAP_FAILED) abort();
    }
    n = ((n ? n : 1) + 255) & ~(size_t)255;
    for (int i = 0; i < g_nblocks; ++i)
        if (g_blocks[i].is_free && g_blocks[i].n == n) {
            g_blocks[i].is_free = 0;
            *p = g_arena + g_blocks[i].off;
            zero((char*)*p, n);
            return 0;
        }
    if (n >= BIG) g_top = (g_top + 4095) & ~(size_t)4095;
    if (g_nblocks == 8192 || g_top + n > ARENA_BYTES) return 2;
    g_blocks[g_nblocks++] = (block_t){g_top, n, 0};
    *p = g_arena + g_top;
    g_top += n;
    return 0;
}
int hipMallocAsync(void** p, size_t n, void* s) { (void)s; return hipMalloc(p, n); }
int hipFree(void* p) {
    for (int i = 0; p && i < g_nblocks; ++i)
        if (g_arena + g_blocks[i].off == (char*)p) g_blocks[i].is_free = 1;
    return 0;
}
int hipFreeAsync(void* p, void* s) { (void)s; return hipFree(p); }
int hipMemcpyAsync(void* d, const void* s, size_t n, int kind, void* st) {
    (void)st;
    if (kind == 2 && n == 12) memcpy(d, g_absmax, 12); else memcpy(d, s, n);
    return 0;
}
int hipMemsetAsync(void* d, int v, size_t n, void* st) { (void)st; if (v == 0) zero((char*)d, n); else memset(d, v, n); return 0; }
int hipMemsetD32Async(void* d, int v, size_t n, void* st) { (void)st; for (size_t i = 0; i < n; ++i) ((int*)d)[i] = v; return 0; }
int hipStreamSynchronize(void* s) { (void)s; return 0; }
int hipStreamWaitEvent(void* s, void* e, unsigned f) { (void)s; (void)e; (void)f; return 0; }
int hipEventCreateWithFlags(void** e, unsigned f) { (void)f; *e = malloc(8); return 0; }
int hipEventDestroy(void* e) { free(e); return 0; }
int hipEventRecord(void* e, void* s) { (void)e; (void)s; return 0; }
int hipEventSynchronize(void* e) { (void)e; return 0; }
int hipGetDevice(int* d) { *d = 0; return 0; }
int hipDeviceGetAttribute(int* v, int a, int d) {   // every attribute, the CU count among them: HIP_STUB_CUS, or 256
    (void)a; (void)d;
    const char* e = getenv("HIP_STUB_CUS");
    *v = e ? atoi(e) : 256;
    return 0;
}
const char* hipGetErrorString(int e) { (void)e; return "stub"; }
int hipGetLastError(void) { return 0; }

// ---- kernels: the name registered for each host function, the sizes of a kernel's arguments (stub_set_kernel_args: the code object's
// metadata has them, the runtime's launch call does not), and the log of launches since stub_clear ------------------------------------
#define MAX_KERNELS 512
#define MAX_LAUNCHES 64
typedef struct { const void* host; const char* name; int n_args; uint32_t size[16]; } kernel_t;
typedef struct { const char* name; uint64_t geom[7]; size_t n; unsigned char* args; unsigned char* raw; } launch_t;
static kernel_t g_kernels[MAX_KERNELS]; static int g_nkernels;
static launch_t g_launches[MAX_LAUNCHES]; static int g_nlaunches;
void stub_set_kernel_args(const char* name, int n_args, const uint32_t* sizes) {
    for (int i = 0; i < g_nkernels; ++i)
        if (strcmp(g_kernels[i].name, name) == 0) {
            g_kernels[i].n_args = n_args < 16 ? n_args : 0;
            memcpy(g_kernels[i].size, sizes, 4 * (size_t)g_kernels[i].n_args);
        }
}
void stub_clear(void) {
    for (int i = 0; i < g_nlaunches; ++i) { free(g_launches[i].args); free(g_launches[i].raw); }
    g_nlaunches = 0;
}
int stub_launches(void) { return g_nlaunches; }
const char* stub_launch_name(int i) { return g_launches[i].name; }
void stub_launch_geometry(int i, uint64_t* out7) { memcpy(out7, g_launches[i].geom, sizeof(g_launches[i].geom)); }   // grid xyz, block xyz, LDS bytes
size_t stub_launch_args(int i, void* dst, size_t cap) {
    const size_t n = g_launches[i].n < cap ? g_launches[i].n : cap;
    if (n) memcpy(dst, g_launches[i].args, n);
    return g_launches[i].n;
}
// the same bytes as the caller passed them, no pointer replaced (a recorder that knows which words are pointers reads a struct whose
// padding is stack garbage through this: garbage beside a 4-byte field can look like a pointer into the arena)
size_t stub_launch_raw_args(int i, void* dst, size_t cap) {
    const size_t n = g_launches[i].n < cap ? g_launches[i].n : cap;
    if (n) memcpy(dst, g_launches[i].raw, n);
    return g_launches[i].n;
}
int hipLaunchKernel(const void* f, dim3_t g, dim3_t b, void** a, size_t sh, void* st) {
    (void)st;
    if (g_nlaunches == MAX_LAUNCHES) return 0;   // (weight finalisation launches more; nobody reads its log)
    launch_t* L = &g_launches[g_nlaunches++];
    *L = (launch_t){"?", {g.x, g.y, g.z, b.x, b.y, b.z, sh}, 0, NULL, NULL};
    for (int i = 0; i < g_nkernels; ++i) {
        const kernel_t* k = &g_kernels[i];
        if (k->host != f) continue;
        L->name = k->name;
        for (int j = 0; j < k->n_args; ++j) L->n += (k->size[j] + 7u) & ~7u;
        L->args = (unsigned char*)calloc(L->n ? L->n : 1, 1);
        L->raw = (unsigned char*)calloc(L->n ? L->n : 1, 1);
        size_t at = 0;
        for (int j = 0; j < k->n_args; ++j) {
            memcpy(L->args + at, a[j], k->size[j]);
            memcpy(L->raw + at, a[j], k->size[j]);
            for (size_t w = 0; w + 8 <= k->size[j]; w += 8) {
                uint64_t v;
                memcpy(&v, L->args + at + w, 8);
                if (in_arena((const void*)(uintptr_t)v)) { v -= (uint64_t)(uintptr_t)g_arena; memcpy(L->args + at + w, &v, 8); }
            }
            at += (k->size[j] + 7u) & ~7u;
        }
    }
    return 0;
}
int __hipPushCallConfiguration(dim3_t g, dim3_t b, size_t sh, void* st) { g_grid = g; g_block = b; g_shmem = sh; g_stream = st; return 0; }
int __hipPopCallConfiguration(dim3_t* g, dim3_t* b, size_t* sh, void** st) { *g = g_grid; *b = g_block; *sh = g_shmem; *st = g_stream; return 0; }
static void* g_fat;
void** __hipRegisterFatBinary(const void* d) { (void)d; return &g_fat; }
void __hipRegisterFunction(void** m, const void* hf, char* df, const char* dn, unsigned tl, void* a, void* b, void* c, void* d, int* w) {
    (void)m; (void)df; (void)tl; (void)a; (void)b; (void)c; (void)d; (void)w;
    if (g_nkernels < MAX_KERNELS) g_kernels[g_nkernels++] = (kernel_t){hf, dn, 0, {0}};
}
void __hipUnregisterFatBinary(void** m) { (void)m; }
