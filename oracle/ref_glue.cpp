/*
 * ref_glue.cpp -- TEST INFRASTRUCTURE ONLY.  C entries around the reference's CudaRasterizer::Rasterizer::{forward, backward,
 * markVisible} once oracle/ref_build.py has compiled the reference's three rasterizer sources for the host (ref_shim/).
 * Plays the part of the reference's rasterize_points.cu without torch: three buffers handed out through callbacks, zeroed
 * gradient outputs, and read-backs of the forward's state through the reference's OWN ImageState / BinningState /
 * GeometryState::fromChunk (rasterizer_impl.h is included, no layout is restated here).
 *
 * The reference's compositor reads the per-Gaussian features through the `shs` pointer (with M == 1 they are a flat (P, C)
 * array) and ignores colors_precomp; its host wrapper passes both, and so does this file.
 */
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

#include "rasterizer_impl.h"   /* the reference's; found through -I <reference>/cuda_rasterizer */
#include "config.h"

using namespace CudaRasterizer;

extern "C" void ref_shim_set_expf(float (*f)(float)) { ref_shim::expf_impl = f; }

namespace {
struct State {
    int P = 0, W = 0, H = 0, R = 0;
    std::vector<char> geom, binning, img;
    std::vector<int> radii;
};

std::function<char*(size_t)> resizer(std::vector<char>& v)
{
    /* zero-filled like nothing in CUDA is -- the only bytes ever read unwritten are GeometryState::clamped */
    return [&v](size_t n) { v.assign(n, 0); return v.data(); };
}
}  // namespace

extern "C" {

int ref_num_channels(void) { return NUM_CHANNELS; }

/* features: (P, NUM_CHANNELS); background: >= NUM_CHANNELS floats; scales/rotations or cov3D_precomp may be NULL.
 * Returns a handle for ref_state_* / ref_backward / ref_free. */
void* ref_forward(int P, int W, int H, const float* background, const float* means3D, const float* features,
                  const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                  const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
                  float tan_fovx, float tan_fovy, int antialiasing, float* out_color, float* out_invdepth, int* radii)
{
    State* s = new State;
    s->P = P; s->W = W; s->H = H;
    s->R = Rasterizer::forward(resizer(s->geom), resizer(s->binning), resizer(s->img), P, /*D=*/0, /*M=*/1, background, W, H,
                               means3D, /*shs=*/features, /*colors_precomp=*/features, opacities, scales, scale_modifier,
                               rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
                               /*prefiltered=*/false, out_color, out_invdepth, antialiasing != 0, radii, /*debug=*/false);
    s->radii.assign(radii, radii + P);
    return s;
}

int ref_num_rendered(void* h) { return ((State*)h)->R; }

/* n_contrib, final_T: H*W; ranges: tiles*2; point_list: R; per Gaussian: xy P*2, depths P, cov3D P*6, conic_opacity P*4,
 * tiles_touched P, point_offsets P.  Any pointer may be NULL. */
void ref_state_read(void* h, uint32_t* n_contrib, float* final_T, uint32_t* ranges, uint32_t* point_list, float* xy,
                    float* depths, float* cov3D, float* conic_opacity, uint32_t* tiles_touched, uint32_t* point_offsets)
{
    State* s = (State*)h;
    const size_t N = (size_t)s->W * s->H, P = (size_t)s->P;
    const size_t tiles = (size_t)((s->W + BLOCK_X - 1) / BLOCK_X) * ((s->H + BLOCK_Y - 1) / BLOCK_Y);
    char* p = s->img.data();
    ImageState img = ImageState::fromChunk(p, N);
    if (n_contrib) memcpy(n_contrib, img.n_contrib, N * sizeof(uint32_t));
    if (final_T) memcpy(final_T, img.accum_alpha, N * sizeof(float));
    if (ranges) memcpy(ranges, img.ranges, tiles * sizeof(uint2));
    p = s->binning.data();
    BinningState bin = BinningState::fromChunk(p, (size_t)s->R);
    if (point_list && s->R) memcpy(point_list, bin.point_list, (size_t)s->R * sizeof(uint32_t));
    p = s->geom.data();
    GeometryState geom = GeometryState::fromChunk(p, P);
    if (xy) memcpy(xy, geom.means2D, P * sizeof(float2));
    if (depths) memcpy(depths, geom.depths, P * sizeof(float));
    if (cov3D) memcpy(cov3D, geom.cov3D, P * 6 * sizeof(float));
    if (conic_opacity) memcpy(conic_opacity, geom.conic_opacity, P * sizeof(float4));
    if (tiles_touched) memcpy(tiles_touched, geom.tiles_touched, P * sizeof(uint32_t));
    if (point_offsets) memcpy(point_offsets, geom.point_offsets, P * sizeof(uint32_t));
}

/* Every dL_d* output is zeroed here first, as the reference's host wrapper does with torch::zeros.
 * dL_dinvdepths (P) and dL_dout_invdepth (H*W) go together: both set or both NULL.  dL_dsh: P*NUM_CHANNELS scratch. */
void ref_backward(void* h, const float* background, const float* means3D, const float* features, const float* opacities,
                  const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                  const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                  int antialiasing, const float* dL_dout_color, const float* dL_dout_invdepth, float* dL_dmeans2D /*P*3*/,
                  float* dL_dconic /*P*4*/, float* dL_dopacity /*P*/, float* dL_dcolors /*P*C*/, float* dL_dinvdepths /*P*/,
                  float* dL_dmeans3D /*P*3*/, float* dL_dcov3D /*P*6*/, float* dL_dsh /*P*C*/, float* dL_dscales /*P*3*/,
                  float* dL_drotations /*P*4*/)
{
    State* s = (State*)h;
    const size_t P = (size_t)s->P;
    memset(dL_dmeans2D, 0, P * 3 * sizeof(float));
    memset(dL_dconic, 0, P * 4 * sizeof(float));
    memset(dL_dopacity, 0, P * sizeof(float));
    memset(dL_dcolors, 0, P * NUM_CHANNELS * sizeof(float));
    if (dL_dinvdepths) memset(dL_dinvdepths, 0, P * sizeof(float));
    memset(dL_dmeans3D, 0, P * 3 * sizeof(float));
    memset(dL_dcov3D, 0, P * 6 * sizeof(float));
    memset(dL_dsh, 0, P * NUM_CHANNELS * sizeof(float));
    memset(dL_dscales, 0, P * 3 * sizeof(float));
    memset(dL_drotations, 0, P * 4 * sizeof(float));
    Rasterizer::backward(s->P, /*D=*/0, /*M=*/1, s->R, background, s->W, s->H, means3D, /*shs=*/features,
                         /*colors_precomp=*/features, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix,
                         projmatrix, campos, tan_fovx, tan_fovy, s->radii.data(), s->geom.data(), s->binning.data(),
                         s->img.data(), dL_dout_color, dL_dout_invdepth, dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors,
                         dL_dinvdepths, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, antialiasing != 0,
                         /*debug=*/false);
}

void ref_free(void* h) { delete (State*)h; }

void ref_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present)
{
    static_assert(sizeof(bool) == 1, "bool");
    Rasterizer::markVisible(P, const_cast<float*>(means3D), const_cast<float*>(viewmatrix), const_cast<float*>(projmatrix),
                            reinterpret_cast<bool*>(present));
}

}  // extern "C"
