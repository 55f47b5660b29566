// tn_api_mlp.hip -- C-ABI of the shallow MLP, the fused renderer, the samplers and the compositing ops
// (see include/tetranerf_hip.h).  A tn_mlp handle owns the packed forms of one set of weights and the per-call scratch.
#include <algorithm>
#include <cstdio>
#include <memory>

#include "tn_api_common.h"
#include "tn_devbuf.h"
#include "tn_kernels.h"

using tn::DeviceGuard;
using tn::guarded;

struct tn_mlp {
    int device = 0;
    tn::DevBuf<float> pk_plain, pk_gather, pt, enc, grad_scratch, wenc, hterm;
    tn::DevBuf<uint4> blob, blob_bf16, blob_t;
    tn::DevBuf<float> render_scratch;    // per-block hand-over area of tn_render_rays (grown on demand, never shrunk)
    tn::DevBuf<unsigned long long> render_prof;   // TETRANERF_HIP_RENDER_PROFILE=1 (debug): phase ticks of tn_render_rays
    bool packed = false;
    // per-call scratch: grown on demand (blocking hipMalloc, rare), never shrunk; one handle serves one stream at a time
    tn::MlpPacks packs(size_t rays) {
        if (!packed) throw tn::Error("tn_mlp_set_weights must be called first");
        if (enc.n < rays * tn::mlp_enc_floats_per_ray() || hterm.n < rays * 128) {
            const size_t cap = std::max<size_t>(rays + rays / 4, 4096);
            TN_HIP(hipDeviceSynchronize());   // the old scratch may still be in use by queued kernels
            enc.alloc(cap * tn::mlp_enc_floats_per_ray());
            hterm.alloc(cap * 128);
        }
        return tn::MlpPacks{pk_plain.p, pk_gather.p, pt.p, blob.p, wenc.p, hterm.p, enc.p, nullptr, grad_scratch.p, blob_bf16.p, blob_t.p};
    }
    // the partial sums of the parameter gradients: allocated by the first training call of this handle
    void ensure_grad_scratch() {
        if (grad_scratch.p) return;
        TN_HIP(hipDeviceSynchronize());
        grad_scratch.alloc(tn::mlp_param_grad_scratch_floats());
    }
};

namespace {
// NULL = the reference configuration's default: white, training-mode renderer (no clamp)
tn::Background background_of(const tn_rgb_background *b) {
    return b ? tn::Background{b->r, b->g, b->b, b->clamp} : tn::Background{1.f, 1.f, 1.f, 0};
}
tn_mlp *checked_mlp(tn_mlp_t m) {
    if (!m) throw tn::Error("mlp handle is null");
    return m;
}
// inference: the evaluation forwards, which also run in plain bf16; everything else (training forward, tn_render_rays) does not.
// no_mode_2: the wording of an entry that refuses mode 2 in words of its own
void check_mode(int mode, bool inference = false, const char *no_mode_2 = nullptr) {
    if (inference) {
        if (mode < 0 || mode > 2) throw tn::Error("mlp mode must be 0 (fp32 MFMA), 1 (bf16x3 MFMA) or 2 (plain bf16 MFMA)");
    } else if (mode == 2) {
        throw tn::Error(no_mode_2 ? no_mode_2
                                  : "mlp mode must be 0 (fp32 MFMA) or 1 (bf16x3 MFMA) here: mode 2 (plain bf16 MFMA) is an arithmetic of "
                                    "tn_mlp_forward and tn_mlp_forward_gather only");
    } else if (mode != 0 && mode != 1) {
        throw tn::Error("mlp mode must be 0 (fp32 MFMA) or 1 (bf16x3 MFMA)");
    }
}
// the inference forward of a mode (one signature)
auto forward_of(int mode) {
    return mode == 2 ? tn::launch_mlp_forward_bf16 : mode ? tn::launch_mlp_forward_x3 : tn::launch_mlp_forward;
}
void require(bool all_given) {
    if (!all_given) throw tn::Error("null pointer");
}
// what the training forward saves (the masks aside: the weight gradients do not read them)
void require_saved(const tn_mlp_backward_buffers *b) { require(b->x0 && b->h1 && b->h2 && b->h3 && b->h4); }
// what the dX chain leaves for the weight gradients (d x0 aside: it belongs to the gather adjoint)
void require_chain(const tn_mlp_backward_buffers *b) { require(b->d1 && b->d2 && b->d3 && b->d4 && b->dhead); }
tn::MlpBackwardBuffers training_buffers(const tn_mlp_backward_buffers *b) {
    return tn::MlpBackwardBuffers{{b->x0, b->h1, b->h2, b->h3, b->h4, (unsigned long long *)b->masks},
                                  b->d1, b->d2, b->d3, b->d4, b->dhead, b->dx0};
}
tn::MlpParamGrads checked_grads(const tn_mlp_grads *g) {
    float *const gp[12] = {g->w1, g->b1, g->w2, g->b2, g->w3, g->b3, g->wd, g->bd, g->wh, g->bh, g->wr, g->br};
    for (float *p : gp) require(p);
    return tn::MlpParamGrads{gp[0], gp[1], gp[2], gp[3], gp[4], gp[5], gp[6], gp[7], gp[8], gp[9], gp[10], gp[11]};
}
// The training stages, one host path each.  listed: slot i < n of the call is sample live[i] of n_samples (the _indexed
// entries); otherwise slot i is sample i and n_samples = n.  -> the rays of the call; the two forms word the condition differently
size_t checked_rays(bool listed, size_t n, size_t n_samples, uint32_t samples_per_ray) {
    if (!listed) {
        if (samples_per_ray == 0 || n % samples_per_ray != 0) throw tn::Error("n must be a multiple of samples_per_ray");
    } else {
        if (samples_per_ray == 0 || n_samples == 0 || n_samples % samples_per_ray != 0)
            throw tn::Error("n_samples must be a positive multiple of samples_per_ray");
        if (n_samples >= 0xFFFFFFFFull || n >= 0xFFFFFFFFull) throw tn::Error("too many samples for one call");
    }
    return n_samples / samples_per_ray;
}

int forward_gather(tn_mlp_t mlp, bool listed, size_t n, uint32_t samples_per_ray, const uint32_t *live, const uint32_t *live_count,
                   const uint32_t *vertex_indices, const float *barycentric, const float *field_vm, const float *dirs, int mode,
                   float *sigma, float *rgb, const float *ray_head_bias, const uint32_t *count, void *stream_) {
    return guarded([&] {
        tn_mlp *m = checked_mlp(mlp);
        check_mode(mode, !listed, "mlp_forward_gather_indexed: mlp mode must be 0 (fp32 MFMA) or 1 (bf16x3 MFMA): the plain-bf16 kernel "
                                  "(mode 2) has no indexed form");
        if (n == 0) return;
        require(vertex_indices && barycentric && field_vm && sigma && (!rgb || dirs) && (!listed || (live && live_count)));
        if (samples_per_ray == 0 || n % samples_per_ray != 0) throw tn::Error("n must be a multiple of samples_per_ray");
        if (listed && n >= 0xFFFFFFFFull) throw tn::Error("too many samples for one call");
        DeviceGuard g(m->device);
        const size_t rays = n / samples_per_ray;
        tn::MlpPacks pk = m->packs(rays);
        pk.ray_bias = rgb ? ray_head_bias : nullptr;
        if (listed)
            tn::launch_mlp_forward_indexed(n, samples_per_ray, rays, live, live_count, vertex_indices, barycentric, field_vm, dirs, pk, mode,
                                           sigma, rgb, (hipStream_t)stream_, count);
        else
            forward_of(mode)(n, samples_per_ray, rays, nullptr, vertex_indices, barycentric, field_vm, dirs, pk, sigma, rgb,
                             (hipStream_t)stream_, count);
        TN_HIP(hipGetLastError());
    });
}

int forward_train(tn_mlp_t mlp, bool listed, size_t n, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live,
                  const uint32_t *vertex_indices, const float *barycentric, const float *field_vm, const float *dirs, int mode,
                  float *sigma, float *rgb, const tn_mlp_backward_buffers *b, const float *ray_head_bias, void *stream_) {
    return guarded([&] {
        tn_mlp *m = checked_mlp(mlp);
        check_mode(mode, false, !listed ? nullptr
                                        : "mlp_forward_gather_train_indexed: mlp mode must be 0 (fp32 MFMA) or 1 (bf16x3 MFMA): the "
                                          "plain-bf16 kernel (mode 2) has neither a training nor an indexed form");
        if (n == 0) return;
        require(vertex_indices && barycentric && field_vm && dirs && sigma && rgb && b && (!listed || live));
        require_saved(b);
        require(b->masks);
        const size_t rays = checked_rays(listed, n, n_samples, samples_per_ray);
        DeviceGuard g(m->device);
        tn::MlpPacks pk = m->packs(rays);
        pk.ray_bias = ray_head_bias;
        if (listed)
            tn::launch_mlp_forward_train_indexed(n, n_samples, samples_per_ray, live, vertex_indices, barycentric, field_vm, dirs, pk, mode,
                                                 sigma, rgb, training_buffers(b), (hipStream_t)stream_);
        else
            (mode ? tn::launch_mlp_forward_x3_train : tn::launch_mlp_forward_train)(
                n, samples_per_ray, rays, vertex_indices, barycentric, field_vm, dirs, pk, sigma, rgb, training_buffers(b),
                (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

// (runs unchanged on the compact columns of a listed forward: there is no listed form)
int backward(tn_mlp_t mlp, size_t n, const float *sigma, const float *rgb, const float *d_sigma, const float *d_rgb,
             const tn_mlp_backward_buffers *b, int mode, void *stream_) {
    return guarded([&] {
        tn_mlp *m = checked_mlp(mlp);
        check_mode(mode);
        if (n == 0) return;
        require(b && sigma && rgb && d_sigma && d_rgb);
        require(b->masks && b->dx0);
        require_chain(b);
        DeviceGuard g(m->device);
        (mode ? tn::launch_mlp_backward_x3 : tn::launch_mlp_backward)(n, sigma, rgb, m->packs(0), d_sigma, d_rgb, training_buffers(b),
                                                                      (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

// d_ray_head_bias covers all rays of the call, so a listed call returns early on n_samples == 0, not on an empty list: an empty
// list still writes the zeros, and reads neither the list nor d4
int ray_head_grad(bool listed, size_t n, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live,
                  const tn_mlp_backward_buffers *b, float *d_ray_head_bias, void *stream_) {
    return guarded([&] {
        if (n_samples == 0) return;
        const bool reads = !listed || n;
        require(d_ray_head_bias && (!reads || (b && b->d4 && (!listed || live))));
        if (samples_per_ray == 0 || n_samples % samples_per_ray != 0)
            throw tn::Error(listed ? "n_samples must be a multiple of samples_per_ray" : "n must be a multiple of samples_per_ray");
        if (listed) {
            if (n_samples >= 0xFFFFFFFFull || n >= 0xFFFFFFFFull) throw tn::Error("too many samples for one call");
            tn::launch_ray_head_grad_indexed(n, n_samples, samples_per_ray, live, reads ? b->d4 : nullptr, d_ray_head_bias,
                                             (hipStream_t)stream_);
        } else {
            tn::launch_ray_head_grad(n, samples_per_ray, b->d4, d_ray_head_bias, (hipStream_t)stream_);
        }
        TN_HIP(hipGetLastError());
    });
}

int param_grads(tn_mlp_t mlp, bool listed, size_t n, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live, const float *dirs,
                const tn_mlp_backward_buffers *b, const tn_mlp_grads *grads, int mode, void *stream_) {
    return guarded([&] {
        tn_mlp *m = checked_mlp(mlp);
        check_mode(mode);
        if (n == 0) return;   // (grads are accumulated into: untouched)
        require(b && grads && dirs && (!listed || live));
        const size_t rays = checked_rays(listed, n, n_samples, samples_per_ray);
        const tn::MlpParamGrads pg = checked_grads(grads);
        require_saved(b);
        require_chain(b);
        DeviceGuard g(m->device);
        m->ensure_grad_scratch();
        const tn::MlpPacks pk = m->packs(rays);
        if (listed)
            tn::launch_mlp_param_grads_indexed(n, n_samples, samples_per_ray, live, dirs, pk, training_buffers(b), pg, mode,
                                               (hipStream_t)stream_);
        else
            (mode ? tn::launch_mlp_param_grads_x3 : tn::launch_mlp_param_grads)(n, samples_per_ray, dirs, pk, training_buffers(b), pg,
                                                                                (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}
}  // namespace

extern "C" {

int tn_mlp_create(int device, tn_mlp_t *out) {
    return guarded([&] {
        if (!out) throw tn::Error("out is null");
        int count = 0;
        TN_HIP(hipGetDeviceCount(&count));
        if (device < 0 || device >= count) throw tn::Error("The device argument must be a CUDA device.");
        DeviceGuard g(device);
        auto m = std::make_unique<tn_mlp>();
        m->device = device;
        m->pk_plain.alloc(tn::mlp_pack_floats());
        m->pk_gather.alloc(tn::mlp_pack_floats());
        m->pt.alloc(tn::mlp_backward_pack_floats());
        m->blob.alloc(tn::mlp_x3_blob_u4());
        m->blob_bf16.alloc(tn::mlp_bf16_blob_u4());
        m->blob_t.alloc(tn::mlp_x3_t_blob_u4());
        m->wenc.alloc(128 * 28);
        *out = m.release();
    });
}

int tn_mlp_destroy(tn_mlp_t mlp) {
    return guarded([&] {
        if (!mlp) return;
        DeviceGuard g(mlp->device);
        (void)hipDeviceSynchronize();
        delete mlp;
    });
}

int tn_mlp_set_weights(tn_mlp_t mlp, const tn_mlp_weights *w, void *stream_) {
    return guarded([&] {
        tn_mlp *m = checked_mlp(mlp);
        if (!w) throw tn::Error("null pointer");
        const float *const all[12] = {w->w1, w->b1, w->w2, w->b2, w->w3, w->b3, w->wd, w->bd, w->wh, w->bh, w->wr, w->br};
        for (const float *x : all) if (!x) throw tn::Error("null weight pointer");
        DeviceGuard g(m->device);
        hipStream_t stream = (hipStream_t)stream_;
        tn::MlpWeights mw{w->w1, w->b1, w->w2, w->b2, w->w3, w->b3, w->wd, w->bd, w->wh, w->bh, w->wr, w->br};
        tn::launch_mlp_pack(mw, m->pk_plain.p, false, stream);
        tn::launch_mlp_pack(mw, m->pk_gather.p, true, stream);
        tn::launch_mlp_pack_t(mw, m->pt.p, stream);
        tn::launch_mlp_pack_x3(mw, m->blob.p, stream);
        tn::launch_mlp_pack_bf16(m->blob.p, m->blob_bf16.p, stream);
        tn::launch_mlp_pack_x3_t(mw, m->blob_t.p, stream);
        tn::launch_pack_wenc(mw, m->wenc.p, stream);
        TN_HIP(hipGetLastError());
        m->packed = true;
    });
}

int tn_mlp_forward(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const float *feats, const float *dirs, int mode,
                   float *sigma, float *rgb, void *stream_) {
    return guarded([&] {
        tn_mlp *m = checked_mlp(mlp);
        check_mode(mode, true);
        if (n == 0) return;
        if (!feats || !sigma || (rgb && !dirs)) throw tn::Error("null pointer");
        if (samples_per_ray == 0 || n % samples_per_ray != 0) throw tn::Error("n must be a multiple of samples_per_ray");
        DeviceGuard g(m->device);
        const size_t rays = n / samples_per_ray;
        forward_of(mode)(
            n, samples_per_ray, rays, feats, nullptr, nullptr, nullptr, dirs, m->packs(rays), sigma, rgb, (hipStream_t)stream_, nullptr);
        TN_HIP(hipGetLastError());
    });
}

int tn_mlp_forward_gather(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const uint32_t *vertex_indices,
                          const float *barycentric, const float *field_vm, const float *dirs, int mode, float *sigma,
                          float *rgb, const float *ray_head_bias, const uint32_t *count, void *stream_) {
    return forward_gather(mlp, false, n, samples_per_ray, nullptr, nullptr, vertex_indices, barycentric, field_vm, dirs, mode, sigma, rgb,
                          ray_head_bias, count, stream_);
}

int tn_render_rays(tn_mlp_t mlp, uint32_t M, const uint32_t *num_visited, const float *hit_distances, const float *barycentric,
                   const uint32_t *vertex_indices, const uint32_t *ray_index, const uint32_t *count, size_t num_hit_rays_max,
                   uint32_t num_samples, uint32_t num_fine, int biased, const float *linspace, const float *u_table,
                   float histogram_padding, float eps, const float *field_vm, const float *dirs,
                   const tn_rgb_background *background, float *out_rgb, float *out_acc, float *out_depth,
                   const float *ray_head_bias, void *stream_) {
    return tn_render_rays_ex(mlp, M, num_visited, hit_distances, barycentric, vertex_indices, ray_index, count, num_hit_rays_max,
                             num_samples, num_fine, biased, linspace, u_table, histogram_padding, eps, field_vm, dirs, background,
                             out_rgb, out_acc, out_depth, ray_head_bias, 0, stream_);
}

int tn_render_rays_ex(tn_mlp_t mlp, uint32_t M, const uint32_t *num_visited, const float *hit_distances, const float *barycentric,
                      const uint32_t *vertex_indices, const uint32_t *ray_index, const uint32_t *count, size_t num_hit_rays_max,
                      uint32_t num_samples, uint32_t num_fine, int biased, const float *linspace, const float *u_table,
                      float histogram_padding, float eps, const float *field_vm, const float *dirs,
                      const tn_rgb_background *background, float *out_rgb, float *out_acc, float *out_depth,
                      const float *ray_head_bias, int mode, void *stream_) {
    return guarded([&] {
        tn_mlp *m = checked_mlp(mlp);
        check_mode(mode);
        if (num_hit_rays_max == 0) return;
        if (!num_visited || !hit_distances || !barycentric || !vertex_indices || !ray_index || !linspace || !field_vm || !dirs ||
            !out_rgb || !out_acc || !out_depth || (num_fine && !u_table))
            throw tn::Error("null pointer");
        if (num_samples == 0) throw tn::Error("num_samples must be positive");
        if (num_hit_rays_max >= 0xFFFFFFFFull) throw tn::Error("too many rays for one call");
        if ((size_t)num_samples + num_fine + 2 > 8192) throw tn::Error("render_rays: too many samples per ray");
        DeviceGuard g(m->device);
        if (!m->packed) throw tn::Error("tn_mlp_set_weights must be called first");
        const unsigned grid = 256;   // one persistent 8-wave block per CU (tn_render_rays.hip)
        tn::RenderRaysLayout L{};
        const size_t need = tn::render_rays_scratch_floats(num_hit_rays_max, num_samples, num_fine, ray_head_bias != nullptr, grid, L);
        if (m->render_scratch.n < need) {
            TN_HIP(hipDeviceSynchronize());   // the old scratch may still be in use by queued kernels
            m->render_scratch.alloc(need + need / 8);
        }
        // debug aid: TETRANERF_HIP_RENDER_PROFILE=1 prints where the persistent kernel's blocks spent their time, per call
        // (a stream synchronisation per call: for profiling runs only)
#if defined(TN_RENDER_DIAG) && TN_RENDER_DIAG
        static const bool profile = tn::env_flag("TETRANERF_HIP_RENDER_PROFILE", false);   // diagnostic builds only (tn_render_rays.hip)
#else
        constexpr bool profile = false;
#endif
        if (profile) {
            if (!m->render_prof.p) m->render_prof.alloc(8);
            TN_HIP(hipMemsetAsync(m->render_prof.p, 0, 8 * sizeof(unsigned long long), (hipStream_t)stream_));
        }
        tn::launch_render_rays(num_visited, hit_distances, barycentric, vertex_indices, M, ray_index, count, num_hit_rays_max, num_samples,
                               num_fine, biased != 0, linspace, u_table, histogram_padding, eps, field_vm, dirs, ray_head_bias, m->packs(0),
                               background_of(background), out_rgb, out_acc, out_depth, m->render_scratch.p, L, grid, (hipStream_t)stream_,
                               profile ? m->render_prof.p : nullptr, mode);
        TN_HIP(hipGetLastError());
        if (profile) {
            unsigned long long h[8];
            TN_HIP(hipStreamSynchronize((hipStream_t)stream_));
            TN_HIP(hipMemcpy(h, m->render_prof.p, sizeof h, hipMemcpyDeviceToHost));
            const double nb = h[5] ? (double)h[5] : 1.0, us = 0.01;   // 100 MHz ticks -> microseconds, mean per working block
            fprintf(stderr, "[tn_render_rays] S=%u fine=%u rays<=%zu blocks=%llu  mean us per block: sample+match %.1f | mlp density %.1f | "
                            "weights+pdf+match %.1f | mlp full %.1f | composite %.1f\n", num_samples, num_fine, num_hit_rays_max,
                    h[5], h[0] * us / nb, h[1] * us / nb, h[2] * us / nb, h[3] * us / nb, h[4] * us / nb);
        }
    });
}

int tn_mlp_forward_gather_train(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const uint32_t *vertex_indices,
                                const float *barycentric, const float *field_vm, const float *dirs, float *sigma, float *rgb,
                                const tn_mlp_backward_buffers *b, const float *ray_head_bias, void *stream_) {
    return forward_train(mlp, false, n, n, samples_per_ray, nullptr, vertex_indices, barycentric, field_vm, dirs, 0, sigma, rgb, b,
                         ray_head_bias, stream_);
}

int tn_mlp_forward_gather_train_ex(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const uint32_t *vertex_indices,
                                   const float *barycentric, const float *field_vm, const float *dirs, int mode, float *sigma,
                                   float *rgb, const tn_mlp_backward_buffers *b, const float *ray_head_bias, void *stream_) {
    return forward_train(mlp, false, n, n, samples_per_ray, nullptr, vertex_indices, barycentric, field_vm, dirs, mode, sigma, rgb, b,
                         ray_head_bias, stream_);
}

int tn_mlp_backward(tn_mlp_t mlp, size_t n, const float *sigma, const float *rgb, const float *d_sigma, const float *d_rgb,
                    const tn_mlp_backward_buffers *b, void *stream_) {
    return backward(mlp, n, sigma, rgb, d_sigma, d_rgb, b, 0, stream_);
}

int tn_mlp_backward_ex(tn_mlp_t mlp, size_t n, const float *sigma, const float *rgb, const float *d_sigma, const float *d_rgb,
                       const tn_mlp_backward_buffers *b, int mode, void *stream_) {
    return backward(mlp, n, sigma, rgb, d_sigma, d_rgb, b, mode, stream_);
}

int tn_mlp_ray_head_grad(size_t n, uint32_t samples_per_ray, const tn_mlp_backward_buffers *b, float *d_ray_head_bias,
                         void *stream_) {
    return ray_head_grad(false, n, n, samples_per_ray, nullptr, b, d_ray_head_bias, stream_);
}

int tn_mlp_param_grads(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const float *dirs, const tn_mlp_backward_buffers *b,
                       const tn_mlp_grads *grads, void *stream_) {
    return param_grads(mlp, false, n, n, samples_per_ray, nullptr, dirs, b, grads, 0, stream_);
}

int tn_mlp_param_grads_ex(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const float *dirs, const tn_mlp_backward_buffers *b,
                          const tn_mlp_grads *grads, int mode, void *stream_) {
    return param_grads(mlp, false, n, n, samples_per_ray, nullptr, dirs, b, grads, mode, stream_);
}

int tn_compact_hits(size_t num_rays, const uint32_t *num_visited, uint32_t *order, uint32_t *count, uint32_t *padded,
                    uint32_t *scratch, size_t scratch_len, void *stream_) {
    return guarded([&] {
        if (!num_visited || !order || !count || !scratch) throw tn::Error("null pointer");
        if (num_rays >= 0xFFFFFFFFull) throw tn::Error("too many rays for one call");
        if (scratch_len < tn::compact_scratch_u32(num_rays)) throw tn::Error("compact_hits: scratch too small (2 * ceil(num_rays / 2048) uint32)");
        tn::launch_compact_hits(num_rays, num_visited, order, count, padded, scratch, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_occupancy_update(uint32_t num_cells, size_t n, const uint32_t *cells, const float *sigma, float decay, float *occupancy,
                        uint32_t samples_per_ray, const uint32_t *count, void *stream_) {
    return guarded([&] {
        if (num_cells == 0) return;
        if (!occupancy || (n && (!cells || !sigma))) throw tn::Error("null pointer");
        if (count && samples_per_ray == 0) throw tn::Error("occupancy_update: a device-side ray count needs samples_per_ray");
        tn::launch_occupancy_update(num_cells, n, cells, sigma, decay, occupancy, samples_per_ray, count, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_cull_samples(size_t n, uint32_t samples_per_ray, const uint32_t *cells, const float *occupancy, uint32_t num_cells,
                    float threshold, uint32_t *live, uint32_t *live_count, float *sigma, float *rgb, uint32_t *scratch,
                    size_t scratch_len, const uint32_t *count, void *stream_) {
    return guarded([&] {
        if (!live_count || !scratch) throw tn::Error("null pointer");
        if (n && (!cells || !live || !sigma || (num_cells && !occupancy))) throw tn::Error("null pointer");
        if (n >= 0xFFFFFFFFull) throw tn::Error("too many samples for one call");
        if (count && samples_per_ray == 0) throw tn::Error("cull_samples: a device-side ray count needs samples_per_ray");
        if (scratch_len < tn::cull_scratch_u32(n)) throw tn::Error("cull_samples: scratch too small (ceil(n / 1024) + 1 uint32)");
        tn::launch_cull_samples(n, samples_per_ray, cells, occupancy, num_cells, threshold, live, live_count, sigma, rgb, scratch, count,
                                (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_mlp_forward_gather_indexed(tn_mlp_t mlp, size_t n_max, uint32_t samples_per_ray, const uint32_t *live,
                                  const uint32_t *live_count, const uint32_t *vertex_indices, const float *barycentric,
                                  const float *field_vm, const float *dirs, int mode, float *sigma, float *rgb,
                                  const float *ray_head_bias, const uint32_t *count, void *stream_) {
    return forward_gather(mlp, true, n_max, samples_per_ray, live, live_count, vertex_indices, barycentric, field_vm, dirs, mode, sigma, rgb,
                          ray_head_bias, count, stream_);
}

int tn_mlp_forward_gather_train_indexed(tn_mlp_t mlp, size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live,
                                        const uint32_t *vertex_indices, const float *barycentric, const float *field_vm,
                                        const float *dirs, int mode, float *sigma, float *rgb, const tn_mlp_backward_buffers *b,
                                        const float *ray_head_bias, void *stream_) {
    return forward_train(mlp, true, n_live, n_samples, samples_per_ray, live, vertex_indices, barycentric, field_vm, dirs, mode, sigma, rgb,
                         b, ray_head_bias, stream_);
}

int tn_mlp_param_grads_indexed(tn_mlp_t mlp, size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live,
                               const float *dirs, const tn_mlp_backward_buffers *b, const tn_mlp_grads *grads, int mode, void *stream_) {
    return param_grads(mlp, true, n_live, n_samples, samples_per_ray, live, dirs, b, grads, mode, stream_);
}

int tn_mlp_ray_head_grad_indexed(size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live,
                                 const tn_mlp_backward_buffers *b, float *d_ray_head_bias, void *stream_) {
    return ray_head_grad(true, n_live, n_samples, samples_per_ray, live, b, d_ray_head_bias, stream_);
}

int tn_compact_rows(uint32_t words_per_row, size_t n_live, const uint32_t *live, const void *src, void *dst, void *stream_) {
    return guarded([&] {
        if (words_per_row != 1 && words_per_row != 3 && words_per_row != 4) throw tn::Error("compact_rows: rows of 1, 3 or 4 32-bit words");
        if (n_live == 0) return;
        if (!live || !src || !dst) throw tn::Error("null pointer");
        tn::launch_compact_rows((int)words_per_row, n_live, live, src, dst, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_sample_coarse(size_t num_hit_rays, uint32_t num_samples, uint32_t M, const uint32_t *ray_index, const uint32_t *num_visited,
                     const float *hit_distances, const float *linspace, const float *t_rand, int biased, float *edges,
                     float *near_far, const uint32_t *count, void *stream_) {
    return guarded([&] {
        if (num_hit_rays == 0) return;
        if (!ray_index || !num_visited || !hit_distances || !linspace || !edges || !near_far) throw tn::Error("null pointer");
        if (num_samples == 0) throw tn::Error("num_samples must be positive");
        tn::launch_sample_coarse(num_hit_rays, num_samples, M, ray_index, num_visited, hit_distances, linspace, t_rand, biased != 0,
                                 edges, near_far, (hipStream_t)stream_, count);
        TN_HIP(hipGetLastError());
    });
}

int tn_sample_pdf(size_t num_hit_rays, uint32_t num_samples, uint32_t num_fine, const float *edges, const float *weights,
                  const float *near_far, const float *u_table, const float *u_rand, float histogram_padding, float eps,
                  float *edges_out, const uint32_t *count, void *stream_) {
    return guarded([&] {
        if (num_hit_rays == 0) return;
        if (!edges || !weights || !near_far || !u_table || !edges_out) throw tn::Error("null pointer");
        if (num_samples == 0) throw tn::Error("num_samples must be positive");
        tn::launch_sample_pdf(num_hit_rays, num_samples, num_fine, edges, weights, near_far, u_table, u_rand, histogram_padding, eps,
                              edges_out, (hipStream_t)stream_, count);
        TN_HIP(hipGetLastError());
    });
}

int tn_sample_live(size_t num_hit_rays, uint32_t num_samples, uint32_t M, const uint32_t *ray_index, const uint32_t *num_visited,
                   const uint32_t *visited, const float *hit_distances, const float *occupancy, uint32_t num_cells, float threshold,
                   const float *linspace, const float *t_rand, float *s_edges, float *near_far_live, const uint32_t *count, void *stream_) {
    return guarded([&] {
        if (num_hit_rays == 0) return;
        if (!ray_index || !num_visited || !visited || !hit_distances || !linspace || !s_edges || !near_far_live || (num_cells && !occupancy))
            throw tn::Error("null pointer");
        if (num_samples == 0) throw tn::Error("num_samples must be positive");
        tn::launch_sample_live(num_hit_rays, num_samples, M, ray_index, num_visited, visited, hit_distances, occupancy, num_cells, threshold,
                               linspace, t_rand, s_edges, near_far_live, (hipStream_t)stream_, count);
        TN_HIP(hipGetLastError());
    });
}

int tn_live_to_distance(size_t num_hit_rays, uint32_t num_values, uint32_t M, const uint32_t *ray_index, const uint32_t *num_visited,
                        const uint32_t *visited, const float *hit_distances, const float *occupancy, uint32_t num_cells, float threshold,
                        const float *values, float *t, uint32_t *slot, const uint32_t *count, void *stream_) {
    return guarded([&] {
        if (num_hit_rays == 0 || num_values == 0) return;
        if (!ray_index || !num_visited || !visited || !hit_distances || !values || !t || !slot || (num_cells && !occupancy))
            throw tn::Error("null pointer");
        tn::launch_live_to_distance(num_hit_rays, num_values, M, ray_index, num_visited, visited, hit_distances, occupancy, num_cells,
                                    threshold, values, t, slot, (hipStream_t)stream_, count);
        TN_HIP(hipGetLastError());
    });
}

int tn_composite_backward(size_t num_rays, uint32_t num_samples, const float *sigma, const float *rgb, const float *edges,
                          const tn_rgb_background *background, const float *d_out_rgb, const float *d_out_acc, float *d_sigma,
                          float *d_rgb, void *stream_) {
    return guarded([&] {
        tn::launch_composite_backward(num_rays, num_samples, sigma, rgb, edges, background_of(background), d_out_rgb, d_out_acc, d_sigma,
                                      d_rgb, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_composite(size_t num_rays, uint32_t num_samples, const float *sigma, const float *rgb, const float *edges,
                 const tn_rgb_background *background, float *out_rgb, float *out_acc, float *out_depth, float *out_weights,
                 const uint32_t *ray_index, const uint32_t *count, void *stream_) {
    return guarded([&] {
        tn::launch_composite(num_rays, num_samples, sigma, rgb, edges, background_of(background), out_rgb, out_acc, out_depth,
                             out_weights, (hipStream_t)stream_, ray_index, count);
        TN_HIP(hipGetLastError());
    });
}

int tn_composite_aux(size_t num_rays, uint32_t num_samples, const float *sigma, const float *edges, float *out_depth_moment,
                     float *out_distortion, float *out_weights, void *stream_) {
    return guarded([&] {
        if (num_rays == 0 || num_samples == 0) return;
        if (!sigma || !edges) throw tn::Error("null pointer");
        tn::launch_composite_aux(num_rays, num_samples, sigma, edges, out_depth_moment, out_distortion, out_weights, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_composite_backward_aux(size_t num_rays, uint32_t num_samples, const float *sigma, const float *rgb, const float *edges,
                              const tn_rgb_background *background, const float *d_out_rgb, const float *d_out_acc,
                              const float *d_out_depth_moment, const float *d_out_distortion, float *d_sigma, float *d_rgb,
                              void *stream_) {
    return guarded([&] {
        if (num_rays == 0 || num_samples == 0) return;
        if (!sigma || !rgb || !edges || !d_sigma || !d_rgb) throw tn::Error("null pointer");
        tn::launch_composite_backward_aux(num_rays, num_samples, sigma, rgb, edges, background_of(background), d_out_rgb, d_out_acc,
                                          d_out_depth_moment, d_out_distortion, d_sigma, d_rgb, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

}  // extern "C"
