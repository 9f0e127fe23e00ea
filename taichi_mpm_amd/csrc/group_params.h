// taichi_mpm_amd/csrc/group_params.h — the per-group material record (material id + parameter row) the constitutive models read.
// Plain C++ without the HIP runtime: shared by the device headers (mpm_math.h, mpm2d_math.h) and by the host builds of the
// same arithmetic under tests/cpp/.  The material ids (MPMHIP_VISCO .. MPMHIP_ELASTIC) and MPMHIP_NPARAM come from the C ABI.
#pragma once
#include <stdint.h>

#include "../../include/mpmhip.h"

namespace mpm {

struct GroupParams {
  float p[MPMHIP_NPARAM];
  int32_t type;
  int32_t pad[3];
};

}  // namespace mpm
