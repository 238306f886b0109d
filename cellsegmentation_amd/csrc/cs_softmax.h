// Softmax over the channel axis of one NCHW pixel, one channel of the result: the arithmetic shared by softmax_ch_fwd_kernel
// (head.hip) and stitch_logits_kernel (detect.hip), which must agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// r: the pixel's channel-0 logit, `stride` floats between channels.  Maximum over the channels, expf of every difference summed
// in channel order, one division.
__device__ __forceinline__ float softmax_channel_at(const float* __restrict__ r, long long stride, int C, int ch) {
    float mx = r[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, r[c * stride]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(r[c * stride] - mx);
    return expf(r[ch * stride] - mx) / se;
}
