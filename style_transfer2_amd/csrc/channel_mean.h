// The channel mean of worker.py:34 (RGB), as preprocess_k subtracts it and emit_k adds it.
#pragma once
#include <hip/hip_runtime.h>

namespace st2 {
static __constant__ float kMean[3] = {123.68f, 116.779f, 103.939f};
}  // namespace st2
