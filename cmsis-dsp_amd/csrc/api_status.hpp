// What the translation units of the C ABI (api.cpp, api_vector.cpp) share.
#pragma once
#include "../../include/arm_math.h"
#include "runtime.hpp"

namespace mi355x {

// status of a batched entry point whose last step returned e; a failure is recorded under `what`
inline arm_status batch_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return ARM_MATH_SUCCESS;
  set_error(e, what);
  return ARM_MATH_ARGUMENT_ERROR;
}

}  // namespace mi355x
