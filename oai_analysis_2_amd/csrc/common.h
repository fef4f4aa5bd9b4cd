// Shared host-side helpers of liboai_hip.so (error reporting, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
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

// exclusive scan of int32 (csrc/mesh.hip): out[i] = sum in[0..i), in place allowed; scratch holds scan_scratch_bytes(n) bytes
size_t scan_scratch_bytes(long long n);
int exclusive_scan_i32(const int* in, int* out, long long n, int* scratch, hipStream_t st);

static inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

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
