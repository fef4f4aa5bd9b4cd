// Shared helpers of liboai_hip.so: error reporting, launch checks, workspaces, and the set rule of the QC kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../../include/oai_hip.h"

namespace oai {

char* error_buffer();                      // thread-local, 512 bytes
int set_error(int code, const char* fmt, ...);

#define OAI_CHECK_ARG(cond, ...)                                            \
    do {                                                                    \
        if (!(cond)) return ::oai::set_error(OAI_ERR_ARG, __VA_ARGS__);     \
    } while (0)

#define OAI_CHECK_HIP(expr)                                                               \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return ::oai::set_error(OAI_ERR_HIP, "%s failed: %s (%s:%d)", #expr,          \
                                    hipGetErrorString(_e), __FILE__, __LINE__);           \
    } while (0)

// after a kernel launch: catches bad launch configurations without synchronising
#define OAI_CHECK_LAUNCH() OAI_CHECK_HIP(hipGetLastError())

#define OAI_CHECK_WORKSPACE(who, have, need)                                                                              \
    do {                                                                                                                  \
        const size_t _have = (have), _need = (need);                                                                      \
        if (_have < _need) return ::oai::set_error(OAI_ERR_WORKSPACE, who ": workspace %zu B < %zu B", _have, _need);     \
    } while (0)

static inline size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// A workspace handed out front to back in 256-byte steps.  The function that fills an entry point's struct of typed pointers with
// take() is also its *_workspace_bytes: over a null base the pointers are null and `off` ends as the size that the same calls need.
struct Ws {
    char* base;
    size_t off = 0;
    explicit Ws(const void* workspace) : base((char*)workspace) {}
    template <class T>
    T* take(size_t count) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += round256(count * sizeof(T));
        return p;
    }
};

// one int from each device address into host[0..), then a stream synchronise: how an entry point reads counts and flags back
int read_ints(int* host, std::initializer_list<const int*> dev, hipStream_t st);

constexpr long long kMaxFaces = 1LL << 28;     // 6 half-edges and 3 flattened corners per face stay below 2^31 - 1 (and the 0x7f7f7f7f fill)
// the sizes the mesh QC and morphometry entry points accept: 0 .. 2^31-2 vertices, 0 .. 2^28 faces
static inline bool mesh_ok(long long n_verts, long long n_faces) { return n_verts >= 0 && n_verts < (1LL << 31) - 1 && n_faces >= 0 && n_faces <= kMaxFaces; }
// the three corners of face f name vertices of the mesh
__device__ __forceinline__ bool face_ok(const int* __restrict__ f, long long n_verts) {
    return f[0] >= 0 && f[0] < n_verts && f[1] >= 0 && f[1] < n_verts && f[2] >= 0 && f[2] < n_verts;
}

// exclusive scan of int32 (csrc/mesh.hip): out[i] = sum in[0..i), in place allowed; scratch holds scan_scratch_bytes(n) bytes
size_t scan_scratch_bytes(long long n);
int exclusive_scan_i32(const int* in, int* out, long long n, int* scratch, hipStream_t st);

// Bucket lists (csrc/mesh.hip): the members of n buckets stored bucket after bucket, bucket b's at list[start[b] .. start[b + 1]).
// count and start hold n + 1 ints each (the last count stays 0, so that start[n] is the total); scratch holds
// scan_scratch_bytes(n + 1) bytes.  bucket_clear, then a kernel that counts with atomicAdd(&count[b], k); bucket_starts scans the
// counts into start and clears count again, which is then the fill cursor of the scatter kernel:
// list[start[b] + atomicAdd(&count[b], k)].
int bucket_clear(int* count, long long n, hipStream_t st);
int bucket_starts(int* count, int* start, long long n, int* scratch, hipStream_t st);

static inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// blocks of a grid-stride launch: one per `threads` items, at least one, at most `cap` (256 CUs x 16 blocks unless the caller says otherwise)
static inline unsigned grid_stride_blocks(long long items, int threads, long long cap = 256LL * 16) {
    const long long blocks = (items + threads - 1) / threads;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// membership of the QC kernels' thresholded sets (oai_mask_overlap, oai_mask_surface): finite and above the threshold
__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool in_set(float v, float thr) { return finite_f32(v) && v > thr; }

// Diagnostics (in-kernel phase stamps, kernel-variant selection by environment -- nothing that changes a result) exist only in
// builds compiled with -DOAI_DIAG (a separate .so that scripts/ load through OAI_LIB_PATH).  The production library never reads
// the environment: diag_env() is the constant default.  The timing ablations with wrong results that rounds 2-5 kept behind
// OAI_DBG / OAI_ABLATE / OAI_EXP switches are written up (profiles/r0*_*.md) and were removed from the sources in round 6.
#ifdef OAI_DIAG
int diag_env(const char* name, int dflt);
#else
static inline int diag_env(const char*, int dflt) { return dflt; }
#endif

}  // namespace oai
