/* Stand-in for <cub/device/device_radix_sort.cuh>. */
#pragma once
#include "../cub.cuh"
