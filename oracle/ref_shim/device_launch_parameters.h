/* Stand-in for <device_launch_parameters.h>: the rasterizer reads its thread position through cooperative groups only. */
#pragma once
#include "ref_shim.h"
