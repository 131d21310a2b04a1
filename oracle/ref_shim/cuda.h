/* Stand-in for <cuda.h>: glm asks for a toolkit version when GLM_FORCE_CUDA is set. */
#pragma once
#ifndef CUDA_VERSION
#define CUDA_VERSION 11080
#endif
