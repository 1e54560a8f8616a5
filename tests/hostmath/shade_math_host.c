/* Host build of csrc/shade_math.h for tests/test_shade_math_host.py: the per-sample forward and backward over M rows. */
#include "../../dreamwaltz-g_amd/csrc/shade_math.h"

/* light_d [3]; albedo, rgbs, grad_rgbs, dalbedo [M, 3]; sigma_fd, dsigma_fd [M, 6] */
void host_shade_forward(unsigned shading, int M, const float* sigma_fd, const float* albedo, const float* light_d, float ratio, float eps,
                        float* normals, float* rgbs) {
    const float omr = (float)(1.0 - (double)ratio);
    for (int i = 0; i < M; ++i) {
        float n[3];
        shade_normal(sigma_fd + 6 * i, eps, n);
        normals[3 * i] = n[0]; normals[3 * i + 1] = n[1]; normals[3 * i + 2] = n[2];
        shade_color(shading, ratio, omr, -light_d[0], -light_d[1], -light_d[2], n[0], n[1], n[2], albedo + 3 * i, 3, rgbs + 3 * i);
    }
}

void host_shade_backward(unsigned shading, int M, const float* sigma_fd, const float* albedo, const float* light_d, float ratio, float eps,
                         const float* grad_rgbs, float* dsigma_fd, float* dalbedo) {
    const float omr = (float)(1.0 - (double)ratio);
    for (int i = 0; i < M; ++i) {
        float da[3] = {0.f, 0.f, 0.f};
        shade_backward(shading, ratio, omr, -light_d[0], -light_d[1], -light_d[2], eps, sigma_fd + 6 * i, albedo + 3 * i, grad_rgbs + 3 * i,
                       dsigma_fd + 6 * i, da);
        dalbedo[3 * i] = da[0]; dalbedo[3 * i + 1] = da[1]; dalbedo[3 * i + 2] = da[2];
    }
}
