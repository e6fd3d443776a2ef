// Host-side helpers for the C-ABI entry points (error reporting, launch geometry).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

// thread-local last-error message (defined in bjx_api.hip)
void bjx_set_error(const char* fmt, ...);

#define BJX_CHECK_ARG(cond, msg) \
  do {                           \
    if (!(cond)) {               \
      bjx_set_error("%s", msg);  \
      return 1;                  \
    }                            \
  } while (0)

static inline int bjx_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    bjx_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return 2;
  }
  return 0;
}

// Row-per-wave kernels: one row per wave (>> 256 CUs worth of workgroups); grid-stride only
// beyond 65536 workgroups (BJX_MAX_BLOCKS overrides).
unsigned bjx_row_grid(int64_t n_rows, int waves_per_block);
// Grid-stride kernels over n_items flat items, `block` threads per workgroup: ceil(n_items / block) clamped to
// [1, 65536].
static inline unsigned bjx_flat_grid(int64_t n_items, int block) {
  const int64_t b = (n_items + block - 1) / block;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// 16-byte vector path is legal when D % 4 == 0 and every non-null pointer is 16-B aligned.
static inline bool bjx_vec4_ptr_ok(const void* p) { return p == nullptr || ((uintptr_t)p & 15u) == 0; }
template <typename... P>
static inline bool bjx_vec4_ok(int64_t D, P... ptrs) {
  return (D % 4 == 0) && (bjx_vec4_ptr_ok((const void*)ptrs) && ...);
}

// Launch of a row-per-wave kernel over ROWS rows with the grid and block of that mapping (bjx_rows.h, which the
// translation unit includes), no shared memory; the kernel's arguments follow.
#define BJX_LAUNCH_ROWS(KERNEL, ROWS, STREAM, ...)                                                \
  hipLaunchKernelGGL(KERNEL, dim3(bjx_row_grid(ROWS, bjx::kWavesPerBlock)), dim3(bjx::kBlock), 0, \
                     (hipStream_t)(STREAM), __VA_ARGS__)
// The same for a kernel template over the sweep width: KERNEL<4> when VEC4_OK (a bjx_vec4_ok result), else KERNEL<1>.
#define BJX_LAUNCH_ROWS_VEC(VEC4_OK, KERNEL, ROWS, STREAM, ...)          \
  do {                                                                   \
    if (VEC4_OK) BJX_LAUNCH_ROWS(KERNEL<4>, ROWS, STREAM, __VA_ARGS__);  \
    else BJX_LAUNCH_ROWS(KERNEL<1>, ROWS, STREAM, __VA_ARGS__);          \
  } while (0)
// The same for a finish with a register-resident form.  KERNEL_RES<NI> holds a 16-byte row of at most 256 * NI floats
// (NI = 1, 2, 4); the two-pass KERNEL<4> takes longer rows and KERNEL<1> those that are not VEC4_OK.
#define BJX_LAUNCH_ROWS_RES(VEC4_OK, D, KERNEL_RES, KERNEL, ROWS, STREAM, ...)                \
  do {                                                                                        \
    if (!(VEC4_OK)) BJX_LAUNCH_ROWS(KERNEL<1>, ROWS, STREAM, __VA_ARGS__);                    \
    else if ((D) <= 256) BJX_LAUNCH_ROWS(KERNEL_RES<1>, ROWS, STREAM, __VA_ARGS__);           \
    else if ((D) <= 512) BJX_LAUNCH_ROWS(KERNEL_RES<2>, ROWS, STREAM, __VA_ARGS__);           \
    else if ((D) <= 1024) BJX_LAUNCH_ROWS(KERNEL_RES<4>, ROWS, STREAM, __VA_ARGS__);          \
    else BJX_LAUNCH_ROWS(KERNEL<4>, ROWS, STREAM, __VA_ARGS__);                               \
  } while (0)

// Store policy of the cache-resident HMC loop kernels (flat leapfrog, gradient-only Gaussian callable): p, q and g
// written through L2 (st4_wt, bjx_device.h).  BJX_LF_POLICY=0 gives plain stores (A/B: tools/README.md); read
// once per process.
static inline bool bjx_lf_write_through() {
  static const bool on = [] {
    const char* e = getenv("BJX_LF_POLICY");
    return e ? atoi(e) != 0 : true;
  }();
  return on;
}
