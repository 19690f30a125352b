// The argument checks of the pfg_seq_* entry points (pfg_seq.hip), apart from the launches and free of HIP, so that a host
// build can run them on their own (tests/seq_host/check_main.cpp, under the sanitizers).  Each returns 0 or the number of
// the clause that refuses, and pfg_seq.hip words the message.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pfg_seq {

constexpr int kMinB = 2, kMaxB = 1 << 20;
constexpr int64_t kMaxDoubles = (int64_t)1 << 40;       // B * row_doubles: 8 TiB, far above any device; keeps the index in 63 bits

enum { OK = 0, BAD_B = 1, BAD_ROW = 2, NULL_ARGUMENT = 3, ALIAS = 4, BAD_STRIDE = 5, BAD_TARGET = 6 };

inline int check_pointers(const void *const *pointers, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!pointers[i]) return NULL_ARGUMENT;
    return OK;
}

// gather and adopt: a population of rows; a and b are the two row arrays, which must differ
inline int check_rows(int B, int64_t row_doubles, const void *const *pointers, size_t n, const void *a, const void *b) {
    if (B < kMinB || B > kMaxB) return BAD_B;
    if (row_doubles < 1 || row_doubles > kMaxDoubles / B) return BAD_ROW;
    if (const int rc = check_pointers(pointers, n)) return rc;
    return a == b ? ALIAS : OK;
}

// reweight: B itself is the kernel's to report (status 4, no other access)
inline int check_reweight(int64_t incr_stride, double ess_target, const void *const *pointers, size_t n) {
    if (const int rc = check_pointers(pointers, n)) return rc;
    if (incr_stride < 0) return BAD_STRIDE;
    return ess_target > 0.0 && ess_target <= 1.0 ? OK : BAD_TARGET;      // (false for a NaN)
}

}  // namespace pfg_seq
