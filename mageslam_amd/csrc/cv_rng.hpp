// cv_rng.hpp — OpenCV 3.4.0's cv::RNG (multiply-with-carry), restated once for every place that
// has to draw what the reference draws: state = (unsigned)state * 4164903690 + (state >> 32);
// uniform(a, b) = a + next() % (b - a), and a == b draws nothing.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MAGE_RNG_HD __host__ __device__ inline
#else
#define MAGE_RNG_HD inline
#endif

namespace mage {

struct CvRng {
    uint64_t state;
    MAGE_RNG_HD explicit CvRng(uint64_t seed) : state(seed ? seed : 0xffffffffull) {}
    MAGE_RNG_HD uint32_t next()
    {
        state = (uint64_t)(uint32_t)state * 4164903690ull + (state >> 32);
        return (uint32_t)state;
    }
    MAGE_RNG_HD int uniform(int a, int b) { return a == b ? a : (int)(next() % (uint32_t)(b - a) + (uint32_t)a); }
};

}  // namespace mage
