// reart_amd/csrc/adam.hip -- torch.optim.Adam's step for the host loops (reart_amd.optim.Adam): every parameter of every
// group in ONE launch.  The tensors of those loops hold 128 to a few thousand floats, so a step is bound by its launches:
// the per-tensor records (pointers, size, and what torch keeps per parameter or per group: step size, second bias
// correction, weight decay, maximize) travel BY VALUE in the kernel arguments -- no pointer table is copied to the device --
// and the grid is flat, sum_k ceil(n_k / 256) blocks, where reart_adam_step_multi covers grid.y x max n.
//
// Arithmetic: float32, every rounding as written (-ffp-contract=off; a fused multiply-add is an explicit fmaf).  The formula is
// torch.optim.Adam's; where it fuses follows torch's own multi-tensor kernels, the path torch takes by default for GPU tensors
// (_foreach_add alpha, _foreach_lerp_, _foreach_mul_, _foreach_addcmul_, _foreach_sqrt, _foreach_div_, _foreach_add_,
// _foreach_addcdiv_ as ATen builds them for gfx950), so that a loop can change optimiser without leaving its trajectory:
//     g = maximize ? -g : g;  g = fma(wd, p, g) (wd != 0)
//     m = fma(1 - beta1, g - m, m);  v = fma(1 - beta2, g * g, v * beta2);  vmax = max(vmax, v) (amsgrad)
//     p = fma(-step_size, m / (sqrt(v or vmax) / bc2_sqrt + eps), p)
// with 1 - beta1, 1 - beta2, step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) formed in double on the
// host and rounded once, as torch forms them.  Measured on the MI355X with torch 2.10: of 64 combinations of these choices
// this one alone gives torch.optim.Adam(foreach=True)'s bits (0 of 15 888 elements differ after one and after six steps over
// amsgrad x weight decay x maximize); torch's single-tensor path differs from both in 1 % of the elements.
//
// Accesses are 4 bytes wide throughout: a parameter may be a view at any element offset, and at these sizes width buys nothing.
#include "common.h"

struct AdamGroupsArgs {
    reart_adam_tensor t[REART_ADAM_MAX_TENSORS];
    int first_block[REART_ADAM_MAX_TENSORS + 1];   // prefix sums of ceil(n / 256); [count] = the grid
    int count;
    float w1, beta2, w2, eps;                      // w1 = 1 - beta1, w2 = 1 - beta2
};

__global__ __launch_bounds__(256) void adam_groups_kernel(AdamGroupsArgs a) {
    // the block's tensor: the last k with first_block[k] <= blockIdx.x (an empty tensor shares its first block with its
    // successor, so the last such k is never empty).  Uniform per block: scalar loads from the kernel arguments.
    const int b = blockIdx.x;
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first_block[mid] <= b) lo = mid; else hi = mid;
    }
    const reart_adam_tensor &s = a.t[lo];
    const int i = (b - a.first_block[lo]) * 256 + (int)threadIdx.x;
    if (i >= s.n) return;
    float g = s.grad[i];
    const float p = s.param[i];
    float m = s.exp_avg[i], v = s.exp_avg_sq[i];
    if (s.maximize) g = -g;
    if (s.weight_decay != 0.f) g = fmaf(s.weight_decay, p, g);
    m = fmaf(a.w1, g - m, m);
    v = fmaf(a.w2, g * g, v * a.beta2);
    s.exp_avg[i] = m;
    s.exp_avg_sq[i] = v;
    float second = v;
    if (s.max_exp_avg_sq) {
        const float vmax = s.max_exp_avg_sq[i];
        second = (v > vmax || v != v) ? v : vmax;      // torch.maximum: a NaN on either side stays
        s.max_exp_avg_sq[i] = second;
    }
    const float denom = sqrtf(second) / s.bias_correction2_sqrt + a.eps;
    s.param[i] = fmaf(-s.step_size, m / denom, p);
}

extern "C" int reart_adam_groups(const reart_adam_tensor *tensors, int count, double beta1, double beta2, double eps,
                                 void *stream) {
    if (count < 0 || count > REART_ADAM_MAX_TENSORS) return REART_ERR_INVALID_ARG;
    if (count > 0 && !tensors) return REART_ERR_INVALID_ARG;
    AdamGroupsArgs a = {};
    int blocks = 0;
    for (int k = 0; k < count; ++k) {
        const reart_adam_tensor &t = tensors[k];
        if (t.n < 0) return REART_ERR_INVALID_ARG;
        if (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return REART_ERR_INVALID_ARG;
        if (!__builtin_isfinite(t.bias_correction2_sqrt) || t.bias_correction2_sqrt <= 0.f) return REART_ERR_INVALID_ARG;
        a.t[k] = t;
        a.first_block[k] = blocks;
        blocks += t.n / 256 + (t.n % 256 != 0);      // at most 32 x 2^23
    }
    if (blocks == 0) return REART_OK;
    a.first_block[count] = blocks;
    a.count = count;
    a.w1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.w2 = (float)(1.0 - beta2); a.eps = (float)eps;
    hipLaunchKernelGGL(adam_groups_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
