/* Stand-in for <cooperative_groups/reduce.h>: included by the rasterizer, nothing of it is used. */
#pragma once
#include "../cooperative_groups.h"
