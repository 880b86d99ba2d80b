// cycload.hpp -- how the kernels of both cycle tests (cycles.hip, cycles4.hip) load a quaternion: the one piece of them
// that needs a HIP type, kept out of cycles.hpp and cycles4.hpp so that those stay plain C++.
#pragma once
#include <hip/hip_runtime.h>

#include "cycles.hpp"

namespace irh {

struct CycDevLoad {  // QQ_k as two 16-byte loads
    const double2 *q;
    __host__ __device__ CycQ operator()(uint32_t k) const {
        const double2 lo = q[2 * (size_t)k], hi = q[2 * (size_t)k + 1];
        return CycQ{lo.x, lo.y, hi.x, hi.y};
    }
};

}  // namespace irh
