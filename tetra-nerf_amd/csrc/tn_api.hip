// tn_api.hip -- the C-ABI of libtetranerf_hip.so (see include/tetranerf_hip.h): the error / version queries and the
// stateless ops.  The tracer handle is in tn_api_tracer.hip, the MLP handle, the renderer and the samplers in tn_api_mlp.hip.
#include "tn_api_common.h"
#include "tn_kernels.h"

namespace tn {

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }

}  // namespace tn

using tn::guarded;

extern "C" {

const char *tn_last_error(void) { return tn::g_last_error.c_str(); }

#define TN_STR2(x) #x
#define TN_STR(x) TN_STR2(x)
const char *tn_version(void) { return "tetranerf_hip 0.6.0 abi " TN_STR(TN_ABI_VERSION) " gfx950"; }
int tn_abi_version(void) { return TN_ABI_VERSION; }

int tn_find_matched_cells_indexed(size_t R, size_t S, size_t M, const uint32_t *ray_index, const uint32_t *num_visited,
                                  const uint32_t *visited, const float *dist, const float *bary, const float *distances,
                                  const uint32_t *verts, uint32_t *cells_out, uint32_t *verts_out, uint8_t *mask_out,
                                  float *bary_out, const uint32_t *count, void *stream_) {
    return guarded([&] {
        if (R == 0 || S == 0) return;
        if (!ray_index) throw tn::Error("ray_index is null");
        if (S >= 0xFFFFFFFFull || M >= 0xFFFFFFFFull) throw tn::Error("num_samples / max_visited_cells too large");
        if (M * 2 * sizeof(float) > 64 * 1024) throw tn::Error("max_visited_cells larger than 8192 is not supported");
        tn::launch_find_matched_cells(R, S, M, num_visited, visited, dist, bary, distances, verts, cells_out,
                                      verts_out, mask_out, bary_out, (hipStream_t)stream_, ray_index, count);
        TN_HIP(hipGetLastError());
    });
}

int tn_find_matched_cells(size_t R, size_t S, size_t M, const uint32_t *num_visited, const uint32_t *visited,
                          const float *dist, const float *bary, const float *distances, const uint32_t *verts,
                          uint32_t *cells_out, uint32_t *verts_out, uint8_t *mask_out, float *bary_out,
                          void *stream_) {
    return guarded([&] {
        if (R == 0 || S == 0) return;
        if (S >= 0xFFFFFFFFull || M >= 0xFFFFFFFFull) throw tn::Error("num_samples / max_visited_cells too large");
        if (M * 2 * sizeof(float) > 64 * 1024) throw tn::Error("max_visited_cells larger than 8192 is not supported");
        tn::launch_find_matched_cells(R, S, M, num_visited, visited, dist, bary, distances, verts, cells_out,
                                      verts_out, mask_out, bary_out, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_interpolate_values(uint32_t D, uint32_t V, uint32_t n, uint32_t Fd, const uint32_t *vi, const float *bc,
                          const float *field, float *result, void *stream_) {
    return guarded([&] {
        tn::launch_interpolate_values(D, V, n, Fd, vi, bc, field, result, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_interpolate_values_backward(uint32_t D, uint32_t V, uint32_t n, uint32_t Fd, const uint32_t *vi,
                                   const float *bc, const float *grad_in, float *field_grad_out, void *stream_) {
    return guarded([&] {
        tn::launch_interpolate_values_backward(D, V, n, Fd, vi, bc, grad_in, false, field_grad_out, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_interpolate_values_backward_rows(uint32_t D, uint32_t V, uint32_t n, uint32_t Fd, const uint32_t *vi,
                                        const float *bc, const float *grad_rows, float *field_grad_out, void *stream_) {
    return guarded([&] {
        tn::launch_interpolate_values_backward(D, V, n, Fd, vi, bc, grad_rows, true, field_grad_out, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

/* vertex-major variants: the caller keeps a [V, Fd] shadow of the field (tn_transpose_f32 makes it, once per field
 * version) -- no per-call O(V) transposition, no temporaries */
int tn_transpose_f32(uint32_t rows, uint32_t cols, const float *in, float *out, void *stream_) {
    return guarded([&] {
        tn::launch_transpose(in, out, rows, cols, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_interpolate_values_vm(uint32_t D, uint32_t n, uint32_t Fd, const uint32_t *vi, const float *bc,
                             const float *field_vm, float *result, void *stream_) {
    return guarded([&] {
        tn::launch_interpolate_values_vm(D, n, Fd, vi, bc, field_vm, result, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_interpolate_values_backward_vm(uint32_t D, uint32_t n, uint32_t Fd, const uint32_t *vi, const float *bc,
                                      const float *grad_rows, float *field_grad_vm, void *stream_) {
    return guarded([&] {
        tn::launch_interpolate_values_backward_vm(D, n, Fd, vi, bc, grad_rows, field_grad_vm, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_interpolate_values_backward_vm_det(uint32_t D, uint32_t V, uint32_t n, uint32_t Fd, const uint32_t *vi, const float *bc,
                                          const float *grad_rows, float *field_grad_vm, void *stream_) {
    return guarded([&] {
        if (n == 0 || Fd == 0) return;
        if (!vi || !bc || !grad_rows || !field_grad_vm) throw tn::Error("null pointer");
        if (V == 0) throw tn::Error("interpolate_values backward (deterministic): the vertex count is 0");
        // vertex ids >= V (TN_EMPTY = an unmatched slot, and any other out-of-range id) sort behind every vertex's run and are
        // skipped; the atomic entry point would write through such an id (the reference does not check either, py_binding.cpp:309-311)
        tn::launch_interpolate_values_backward_vm_det(D, V, n, Fd, vi, bc, grad_rows, field_grad_vm, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

/* position gradients (tn_position_grad.hip): what py_binding.cpp:354 leaves as a TODO and extension/__init__.py:45-68 states in
 * PyTorch; the expressions are in include/tetranerf_hip.h */
int tn_interpolate_values_backward_bary_vm(uint32_t D, uint32_t n, uint32_t Fd, const uint32_t *vi, const float *grad_rows,
                                           const float *field_vm, float *grad_bary, void *stream_) {
    return guarded([&] {
        if (n == 0) return;
        if (!vi || !grad_bary || (Fd && (!grad_rows || !field_vm))) throw tn::Error("null pointer");
        tn::launch_interpolate_values_backward_bary_vm(D, n, Fd, vi, grad_rows, field_vm, grad_bary, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_sample_positions_backward(size_t R, uint32_t S, uint32_t V, const uint32_t *vi, const float *bc, const float *grad_bary,
                                 const float *distances, const float *vertices, float *grad_points, float *grad_origins,
                                 float *grad_directions, float *grad_vertices, void *stream_) {
    return guarded([&] {
        if (R == 0 || S == 0) return;
        if (!grad_points && !grad_origins && !grad_directions && !grad_vertices) return;
        if (!vi || !bc || !grad_bary || !vertices) throw tn::Error("null pointer");
        if (grad_directions && !distances) throw tn::Error("sample_positions backward: grad_directions needs the sample distances");
        if (R > 0xFFFFFFFFull / S) throw tn::Error("sample_positions backward: too many samples");
        tn::launch_sample_positions_backward(R, S, V, vi, bc, grad_bary, distances, vertices, grad_points, grad_origins,
                                             grad_directions, grad_vertices, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_gather_uint32(int elem_size, uint32_t num_values, uint32_t num_indices, const uint32_t *indices,
                     const void *values, void *result, void *stream_) {
    return guarded([&] {
        tn::launch_gather_uint32(elem_size, num_values, num_indices, indices, values, result, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_scatter_ema_uint32(int elem_size, uint32_t num_result, uint32_t num_indices, const uint32_t *indices,
                          double decay, const void *values, void *result, void *stream_) {
    return guarded([&] {
        tn::launch_scatter_ema_uint32(elem_size, num_result, num_indices, indices, decay, values, result, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

/* the RAdam step (tn_optim.hip): what torch.optim.RAdam runs as a chain of element-wise launches; the statement is in
 * include/tetranerf_hip.h */
static tn::RadamHyper radam_hyper(const tn_radam_hyper *hyper) {
    if (!hyper) throw tn::Error("radam step: hyper is null");
    if (hyper->decay_mode < 0 || hyper->decay_mode > 2) throw tn::Error("radam step: decay_mode must be 0, 1 or 2");
    return tn::RadamHyper{hyper->one_minus_beta1, hyper->beta2, hyper->one_minus_beta2, hyper->eps, hyper->decay, hyper->decay_mode};
}

int tn_radam_step_field(uint32_t num_vertices, float *field, const float *grad, float *exp_avg, float *exp_avg_sq, float *shadow_vm,
                        float step_size, int adaptive, const tn_radam_hyper *hyper, void *stream_) {
    return guarded([&] {
        const tn::RadamHyper h = radam_hyper(hyper);
        if (num_vertices == 0) return;
        if (!field || !grad || !exp_avg || !exp_avg_sq) throw tn::Error("radam step: null pointer");
        tn::launch_radam_field(num_vertices, field, grad, exp_avg, exp_avg_sq, shadow_vm, h, step_size, adaptive != 0,
                               (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_radam_step(size_t num_tensors, const tn_radam_tensor *tensors, const tn_radam_hyper *hyper, void *stream_) {
    return guarded([&] {
        const tn::RadamHyper h = radam_hyper(hyper);
        if (num_tensors == 0) return;
        if (!tensors) throw tn::Error("radam step: the tensor table is null");
        // the table of one launch is built from at most RADAM_TABLE entries at a time: no allocation here
        for (size_t i = 0; i < num_tensors; ++i) {      // (all of them before the first launch: a refused call writes nothing)
            const tn_radam_tensor &t = tensors[i];
            if (t.count && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) throw tn::Error("radam step: null pointer");
        }
        tn::RadamTensor part[tn::RADAM_TABLE];
        for (size_t i0 = 0; i0 < num_tensors; i0 += tn::RADAM_TABLE) {
            const size_t k = num_tensors - i0 < tn::RADAM_TABLE ? num_tensors - i0 : tn::RADAM_TABLE;
            for (size_t i = 0; i < k; ++i) {
                const tn_radam_tensor &t = tensors[i0 + i];
                part[i] =tn::RadamTensor{t.param, t.grad, t.exp_avg, t.exp_avg_sq, (uint64_t)t.count, t.step_size, t.adaptive != 0, 0u};
            }
            tn::launch_radam_flat(k, part, h, (hipStream_t)stream_);
            TN_HIP(hipGetLastError());
        }
    });
}

}  // extern "C"
