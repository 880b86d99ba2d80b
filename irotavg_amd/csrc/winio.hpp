// winio.hpp -- how the window kernels (window.hip: the solve, wincov.hip: the uncertainty) move a row of four doubles
// between a caller's strided device matrix and registers. One copy, so that the batched forms of both read the same bytes
// the same way.
#pragma once
#include <hip/hip_runtime.h>

namespace irh {

// 8-byte accesses through (rs, cs); 16-byte ones only for contiguous rows behind a 16-byte aligned pointer (aos: rows16 of
// winbatch.hpp). Never a double4 access: packed offsets and tensor views give no 32-byte alignment.
__device__ __forceinline__ double4 ld_row(const double *p, long long rs, long long cs, long long row, bool aos) {
    if (aos) {
        const double2 *h = reinterpret_cast<const double2 *>(p + 4 * row);
        const double2 a = h[0], b = h[1];
        return make_double4(a.x, a.y, b.x, b.y);
    }
    const double *r = p + row * rs;
    return make_double4(r[0], r[cs], r[2 * cs], r[3 * cs]);
}
__device__ __forceinline__ void st_row(double *p, long long rs, long long cs, long long row, bool aos, const double4 &v) {
    if (aos) {
        double2 *h = reinterpret_cast<double2 *>(p + 4 * row);
        h[0] = make_double2(v.x, v.y);
        h[1] = make_double2(v.z, v.w);
        return;
    }
    double *r = p + row * rs;
    r[0] = v.x;
    r[cs] = v.y;
    r[2 * cs] = v.z;
    r[3 * cs] = v.w;
}

}  // namespace irh
