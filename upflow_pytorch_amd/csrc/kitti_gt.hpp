// Decoding one sample of a KITTI flow PNG's uint16 payload (R = u*64 + 2^15, G = v*64 + 2^15, B = valid), shared by the kernels
// that read the ground truth as the files hold it (score.hip, errmap.hip): ONE spelling, so they agree bit for bit.
#pragma once
#include "common.hpp"

namespace upf {
namespace kitti {

// R or G (the low 16 bits of s) -> a flow component; exact: the host path's float64 decode rounded to fp32
__device__ __forceinline__ float gt_flow(uint32_t s) { return (float)((int)s - 32768) * 0.015625f; }

// B -> the mask as the host path's np.uint8() leaves it (it wraps)
__device__ __forceinline__ int gt_mask(uint32_t s) { return (int)(s & 255u); }

}  // namespace kitti
}  // namespace upf
