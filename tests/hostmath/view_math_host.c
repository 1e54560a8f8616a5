/* Host build of csrc/view_math.h for tests/test_nerf_view_host.py: the per-pixel ray, the mix and the sparsity terms over arrays. */
#include "../../dreamwaltz-g_amd/csrc/view_math.h"

/* c2w [16], intrinsics [9] -> rays_o, rays_d [H W, 3] in the kernel's pixel order */
void host_view_rays(const float* c2w, const float* intrinsics, int H, int W, float* rays_o, float* rays_d) {
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const int n = r * W + c;
            view_ray(c2w, intrinsics, (uint32_t)r, (uint32_t)c, rays_d + 3 * n);
            rays_o[3 * n] = c2w[3]; rays_o[3 * n + 1] = c2w[7]; rays_o[3 * n + 2] = c2w[11];
        }
}

/* image [C, N] planar <- fg [N, C] + (1 - ws [N]) * bg ([C], or [N, C] with per_pixel) */
void host_view_mix(int N, int C, const float* fg, const float* ws, const float* bg, int per_pixel, float* image) {
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < C; ++c) image[c * N + n] = view_mix(fg[C * n + c], ws[n], bg[per_pixel ? C * n + c : c]);
}

/* terms [N, 3] fp32 <- the three per-element terms rounded once; sums [3] <- their fp64 sums in index order; loss [1] fp32;
 * grad [N] fp32 <- d loss / d ws rounded once */
void host_sparsity(int N, const float* ws, double lambda_opacity, double lambda_entropy, double lambda_emptiness, double mult, float* terms,
                   double* sums, float* loss, float* grad) {
    sums[0] = sums[1] = sums[2] = 0.0;
    for (int n = 0; n < N; ++n) {
        double t[3];
        sparsity_terms(ws[n], t);
        for (int k = 0; k < 3; ++k) { terms[3 * n + k] = (float)t[k]; sums[k] += t[k]; }
    }
    loss[0] = (float)sparsity_loss(sums, (double)N, lambda_opacity, lambda_entropy, lambda_emptiness, mult);
    for (int n = 0; n < N; ++n)
        grad[n] = (float)sparsity_derivative(ws[n], sums[0], (double)N, lambda_opacity, lambda_entropy, lambda_emptiness, mult);
}
