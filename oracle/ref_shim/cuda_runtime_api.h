/* Stand-in for <cuda_runtime_api.h>; everything lives in ref_shim.h. */
#pragma once
#include "ref_shim.h"
