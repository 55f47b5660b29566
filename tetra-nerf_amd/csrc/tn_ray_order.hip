// tn_ray_order.hip -- the locality order of a binned trace_rays call (TN_TRACE_BIN_RAYS, include/tetranerf_hip.h):
// the mesh box (at load), a 30-bit key per ray, and a stable radix sort of (key, caller index).  The key is stated once, in
// tetra-nerf_amd/ray_order.py (ray_keys); tn_ray_key.h is that statement operation for operation, so that
// order == argsort(ray_keys, stable) bit for bit (tests/test_bin_rays_gpu.py).
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "tn_kernels.h"

namespace tn {

namespace {

// floats as unsigned integers of the same order (-0 < +0; no NaN gets here)
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
float unordered(uint32_t u) {
    const uint32_t b = (u >> 31) ? (u & 0x7FFFFFFFu) : ~u;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// min / max of the coordinates of the vertices `cells` references: box[0..2] = min, box[3..5] = max, as ordered().  min and
// max are exact, so the device build, the host build and numpy see the same six numbers.  NaN coordinates are skipped.
__global__ __launch_bounds__(256) void k_mesh_box(size_t n, uint32_t V, const uint32_t *__restrict__ cells,
                                                  const float *__restrict__ xyz, uint32_t *__restrict__ box) {
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t v = cells[i];
        if (v >= V) continue;                  // (the builds refuse such a mesh)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = xyz[3 * (size_t)v + k];
            if (f != f) continue;
            const uint32_t u = ordered(f);
            lo[k] = u < lo[k] ? u : lo[k];
            hi[k] = u > hi[k] ? u : hi[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int off = 32; off; off >>= 1) {
            const uint32_t a = (uint32_t)__shfl_xor((int)lo[k], off), b = (uint32_t)__shfl_xor((int)hi[k], off);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&box[k], lo[k]);
            atomicMax(&box[3 + k], hi[k]);
        }
    }
}

// one lane per ray: keys[r] = ray_keys(...)[r] of tetra-nerf_amd/ray_order.py (tn_ray_key.h), iota[r] = r
__global__ __launch_bounds__(256) void k_ray_keys(size_t R, const float *__restrict__ origins, const float *__restrict__ dirs,
                                                  RayKeyBox b, uint32_t *__restrict__ keys, uint32_t *__restrict__ iota) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    keys[r] = ray_key(origins[3 * r], origins[3 * r + 1], origins[3 * r + 2], dirs[3 * r], dirs[3 * r + 1], dirs[3 * r + 2], b);
    iota[r] = (uint32_t)r;
}

}  // namespace

void mesh_box(size_t V, size_t T, const float *xyz, const uint32_t *cells, float lo[3], float hi[3], hipStream_t stream) {
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = 0.f;
    if (!T || !V) return;
    uint32_t *box = nullptr;
    TN_HIP(hipMalloc((void **)&box, 6 * sizeof(uint32_t)));
    uint32_t h[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    hipError_t e = hipMemcpyAsync(box, h, sizeof h, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const size_t n = 4 * T;
        const size_t blocks = std::min<size_t>((n + 255) / 256, 2048);
        hipLaunchKernelGGL(k_mesh_box, dim3((unsigned)blocks), dim3(256), 0, stream, n, (uint32_t)V, cells, xyz, box);
        e = hipMemcpyAsync(h, box, sizeof h, hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(box);
    TN_HIP(e);
    for (int k = 0; k < 3; ++k)
        if (h[k] <= h[3 + k]) { lo[k] = unordered(h[k]); hi[k] = unordered(h[3 + k]); }   // (else: every coordinate NaN)
}

size_t ray_order_temp_bytes(size_t R) {
    size_t bytes = 0;
    TN_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                     (uint32_t *)nullptr, R, 0u, (unsigned)RAY_KEY_BITS, (hipStream_t) nullptr));
    return bytes ? bytes : 1;
}

void launch_ray_order(size_t R, const float *origins, const float *dirs, const RayKeyBox &box, uint32_t *keys, uint32_t *iota,
                      uint32_t *keys_sorted, uint32_t *order, void *temp, size_t temp_bytes, hipStream_t stream) {
    if (R == 0) return;
    hipLaunchKernelGGL(k_ray_keys, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, stream, R, origins, dirs, box, keys, iota);
    TN_HIP(rocprim::radix_sort_pairs(temp, temp_bytes, keys, keys_sorted, iota, order, R, 0u, (unsigned)RAY_KEY_BITS, stream));
}

}  // namespace tn
