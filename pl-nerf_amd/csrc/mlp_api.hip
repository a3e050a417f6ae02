// MLP entry points of the C ABI (include/plnerf_hip.h): argument validation and dispatch on
// the precision mode.  Kernels live in mlp_f32.hip (exact fp32 MFMA), mlp_wgrad.hip (the weight-gradient stage of every
// mode), mlp_h16.hip (the 16-bit-operand MFMA modes, bf16 and IEEE-half elements, plain and 3-term split: ping-pong
// forward and dgrad chain) and mlp_rr.hip (their register-resident forward).
#include <cstdlib>

#include "common.h"
#include "mlp_bwd_plan.h"
#include "mlp_fwd_route.h"
#include "mlp_internal.h"
#include "mlp_layout.h"
#include "mlp_unique_plan.h"
#include "../../include/experimental/plnerf_hip_unique.h"

using namespace plnerf;

namespace {
inline int ns_of(int precision) {
    return (precision == PLNERF_PREC_BF16 || precision == PLNERF_PREC_F16) ? 1
           : (precision == PLNERF_PREC_BF16X3 || precision == PLNERF_PREC_F16X3) ? 2 : 0;
}
inline int f16_of(int precision) { return precision == PLNERF_PREC_F16X3 || precision == PLNERF_PREC_F16; }
inline int elem_of(int precision) { return f16_of(precision) ? route::ELEM_f16 : route::ELEM_bf16; }      // (16-bit modes)
inline bool known(int precision) { return precision >= PLNERF_PREC_FP32 && precision <= PLNERF_PREC_F16; }
// network input widths the padded GEMMs can hold (the reference's defaults are 63 / 27)
inline bool geometry_ok(int input_ch, int input_ch_views) {
    return input_ch >= 1 && input_ch <= lay::PE_K && input_ch_views >= 1 && input_ch_views <= lay::DPE_K;
}
// Forward kernel of the 16-bit modes: `fwd_kernel` is an ABI argument (PLNERF_FWD_KERNEL_AUTO / _RR / _PP; the library
// reads no environment for it); which kernel a call runs on is route::fwd_uses_rr (mlp_fwd_route.h) and nothing else.
// (The one variable the library does read: PLNERF_BWD_COMPACT, impl::bwd_compact at the end of this file.)
inline bool kernel_arg_ok(int k) { return k == PLNERF_FWD_KERNEL_AUTO || k == PLNERF_FWD_KERNEL_RR || k == PLNERF_FWD_KERNEL_PP; }
static_assert(route::FWD_AUTO == PLNERF_FWD_KERNEL_AUTO && route::FWD_RR == PLNERF_FWD_KERNEL_RR && route::FWD_PP == PLNERF_FWD_KERNEL_PP, "");
inline bool use_rr(int precision, bool training, bool embedded, int forced) {      // (16-bit modes)
    return route::fwd_uses_rr(elem_of(precision), ns_of(precision), training, embedded, forced);
}
}  // namespace

// bytes of the weight sections; the 16-byte status block follows them
inline size_t sections_bytes(int precision) {
    if (precision == PLNERF_PREC_FP32) return impl::f32_packed_bytes();
    if (ns_of(precision))
        return impl::h16_packed_bytes(ns_of(precision)) + impl::rr_packed_bytes(ns_of(precision));      // (+ the register-resident section)
    return 0;
}
inline unsigned* status_word(void* packed, int precision) {
    return ns_of(precision) ? (unsigned*)((unsigned char*)packed + sections_bytes(precision)) : nullptr;      // every 16-bit mode
}

inline float* compose_block(const void* packed, int precision) {      // (16-bit modes)
    return (float*)((unsigned char*)const_cast<void*>(packed) + impl::h16_compose_offset(ns_of(precision)));
}

extern "C" size_t plnerf_mlp_packed_bytes(int precision) {
    const size_t n = known(precision) ? sections_bytes(precision) : 0;
    return n ? n + 16 : 0;
}

extern "C" size_t plnerf_mlp_status_offset(int precision) { return known(precision) ? sections_bytes(precision) : 0; }

extern "C" int plnerf_mlp_pack_weights(const float* const* params, int precision, int input_ch,
                                       int input_ch_views, void* packed, plnerf_stream_t stream) {
    if (!params || !packed || !geometry_ok(input_ch, input_ch_views)) return PLNERF_EINVAL;
    if (!known(precision)) return PLNERF_ENOSYS;
    for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
        if (!params[i]) return PLNERF_EINVAL;
    if (!aligned16(params[lay::P_WF]) || !aligned16(params[lay::P_BF])) return PLNERF_EINVAL;      // copied as float4 (mlp_compose.hip)
    if (precision == PLNERF_PREC_FP32) return impl::f32_pack(params, input_ch, input_ch_views, packed, (hipStream_t)stream);
    // 16-bit modes: the composed view layer first (W_c = W_vf W_f, b_c; mlp_layout.h) -- the operand sections are packed from it
    float* cb = compose_block(packed, precision);
    int rc = impl::compose_pack(params, input_ch_views, cb, (hipStream_t)stream);
    if (rc) return rc;
    rc = impl::h16_pack(params, input_ch, input_ch_views, ns_of(precision), f16_of(precision), packed,
                        status_word(packed, precision), (hipStream_t)stream);
    if (rc) return rc;
    void* rr_section = (unsigned char*)packed + impl::h16_packed_bytes(ns_of(precision));
    return f16_of(precision) ? impl::rr_pack_f16(params, input_ch, input_ch_views, ns_of(precision), cb, rr_section, (hipStream_t)stream)
                             : impl::rr_pack_bf16(params, input_ch, input_ch_views, ns_of(precision), cb, rr_section, (hipStream_t)stream);
}

// fp32 mode: fp32 planes; 16-bit MFMA modes: half planes (mlp_layout.h)
extern "C" size_t plnerf_mlp_saved_bytes(int n_rows, int precision) {
    if (!known(precision) || n_rows < 0) return 0;
    if (precision == PLNERF_PREC_FP32) return (size_t)lay::SAVED_PER_ROW * (size_t)n_rows * sizeof(float);
    return (size_t)lay::SVH_BYTES_PER_ROW * lay::sv_rows((size_t)n_rows);      // rows padded to whole workgroup tiles (SV_ROW_PAD)
}

// layout of the 256-wide saved planes the forward of this configuration writes (lay::SV_LAYOUT_*): the backward is
// told, so that whichever forward kernel ran, the weight-gradient stage reads its planes as they are
extern "C" int plnerf_mlp_saved_layout(int precision, int has_embedded, int fwd_kernel) {
    if (!known(precision) || !kernel_arg_ok(fwd_kernel)) return PLNERF_EINVAL;
    if (!ns_of(precision)) return lay::SV_LAYOUT_ROWS;
    return use_rr(precision, true, has_embedded != 0, fwd_kernel) ? lay::SV_LAYOUT_TILED : lay::SV_LAYOUT_ROWS;
}

extern "C" size_t plnerf_mlp_bwd_workspace_bytes(int n_rows, int precision) {
    if (!known(precision) || n_rows < 0) return 0;
    return bwdplan::workspace((size_t)n_rows, ns_of(precision) != 0).total;
}

extern "C" int plnerf_mlp_fwd(const void* packed, int precision, const float* pts, const float* viewdirs,
                              const float* embedded, int input_ch, int input_ch_views, int n_rows,
                              int samples_per_ray, float input_scale, float density_beta, float* raw_out, void* saved,
                              int fwd_kernel, plnerf_stream_t stream) {
    if (!known(precision)) return PLNERF_ENOSYS;
    if (!kernel_arg_ok(fwd_kernel)) return PLNERF_EINVAL;
    if (n_rows < 0 || !geometry_ok(input_ch, input_ch_views) || !(density_beta >= 0.0f) || !(density_beta < 1e6f)) return PLNERF_EINVAL;
    const impl::FwdOpt opt{input_scale, density_beta};
    // the in-kernel encoding: 3 + 6 L position channels (L <= 10) and 3 + 6 M direction channels (M <= 4) -- a prefix of
    // the reference default's 63 | 27 (the unused bands meet zero-padded weights) -- with the encoder's input scale
    if (!embedded && ((input_ch - 3) % 6 != 0 || input_ch < 3 || input_ch > lay::XYZ_CH || (input_ch_views - 3) % 6 != 0 ||
                      input_ch_views < 3 || input_ch_views > lay::DIR_CH || !(input_scale > 0.0f) || !(input_scale < 1e6f)))
        return PLNERF_EINVAL;
    if (n_rows == 0) return PLNERF_OK;
    if (!packed || !raw_out || !aligned16(raw_out)) return PLNERF_EINVAL;      // (raw_out is stored as float4)
    if (!embedded && (!pts || !viewdirs || samples_per_ray < 1)) return PLNERF_EINVAL;
    if (precision == PLNERF_PREC_FP32)
        return impl::f32_fwd(packed, pts, viewdirs, embedded, input_ch, input_ch_views, n_rows, samples_per_ray,
                             opt, raw_out, saved, (hipStream_t)stream);
    if (use_rr(precision, saved != nullptr, embedded != nullptr, fwd_kernel))
        return impl::rr_fwd(elem_of(precision), packed, (const unsigned char*)packed + impl::h16_packed_bytes(ns_of(precision)),
                            ns_of(precision), pts, viewdirs, embedded, input_ch, input_ch_views, n_rows, samples_per_ray,
                            opt, raw_out, saved, status_word(const_cast<void*>(packed), precision), (hipStream_t)stream);
    return impl::h16_fwd(packed, ns_of(precision), f16_of(precision), pts, viewdirs, embedded, input_ch,
                         input_ch_views, n_rows, samples_per_ray, opt, raw_out, saved,
                         status_word(const_cast<void*>(packed), precision), (hipStream_t)stream);
}

// The backward of up to PLNERF_MAX_BWD_JOBS networks that share precision, input widths and density activation (the
// coarse and the fine network of one training step) in ONE launch sequence: one dgrad grid and one main / thin / head /
// reduce launch of the weight-gradient stage cover every job (16-bit modes; the exact-fp32 mode runs the jobs one after
// the other).  plnerf_mlp_bwd is the one-job case.
extern "C" int plnerf_mlp_bwd_multi(int n_jobs, const void* const* packed, int precision, const float* const* g_raw,
                                    const uint32_t* const* g_absmax, const int* n_absmax, int input_ch,
                                    int input_ch_views, const int* n_rows, const void* const* saved, const int* saved_layout,
                                    const float* const* raw_out, float density_beta, void* const* workspace,
                                    float* const* grads, float* const* status_out, plnerf_stream_t stream) {
    if (n_jobs < 1 || n_jobs > PLNERF_MAX_BWD_JOBS) return PLNERF_EINVAL;
    if (!known(precision)) return PLNERF_ENOSYS;
    if (!packed || !g_raw || !n_rows || !saved || !saved_layout || !workspace || !grads) return PLNERF_EINVAL;
    if (!geometry_ok(input_ch, input_ch_views)) return PLNERF_EINVAL;
    if (!(density_beta >= 0.0f) || !(density_beta < 1e6f)) return PLNERF_EINVAL;
    const bool act = density_beta > 0.0f;
    for (int j = 0; j < n_jobs; ++j) {
        if (saved_layout[j] != lay::SV_LAYOUT_ROWS && saved_layout[j] != lay::SV_LAYOUT_TILED) return PLNERF_EINVAL;
        if (saved_layout[j] == lay::SV_LAYOUT_TILED && !ns_of(precision)) return PLNERF_EINVAL;
        if (!packed[j] || !g_raw[j] || !saved[j] || !workspace[j] || n_rows[j] < 1) return PLNERF_EINVAL;
        if (act && (!raw_out || !raw_out[j])) return PLNERF_EINVAL;
        if (!aligned16(g_raw[j]) || (act && !aligned16(raw_out[j]))) return PLNERF_EINVAL;      // read as float4
        for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
            if (!grads[j * PLNERF_N_PARAM_TENSORS + i]) return PLNERF_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    // The job's workspace, carved by the one layout (mlp_bwd_plan.h).  The exact-fp32 mode runs each job to its end in
    // turn; the 16-bit modes collect the jobs for the launches they share.
    const bool half = ns_of(precision) != 0;
    impl::DgradJob dj[PLNERF_MAX_BWD_JOBS];
    impl::WgradJob wj[PLNERF_MAX_BWD_JOBS];
    impl::LiveJob lj[PLNERF_MAX_BWD_JOBS];      // 16-bit modes: the networks whose backward runs over the live rows only (mlp_bwd_plan.h)
    int n_live_jobs = 0;
    bool compact = half;      // (every network of the call, or none: they share the weight-gradient launches)
    for (int j = 0; j < n_jobs; ++j) compact = compact && impl::bwd_compact(n_rows[j]);
    for (int j = 0; j < n_jobs; ++j) {
        const bwdplan::Workspace lo = bwdplan::workspace((size_t)n_rows[j], half);
        unsigned char* ws = (unsigned char*)workspace[j];
        unsigned* gmax = half ? (unsigned*)(ws + lo.gmax) : nullptr;      // (fp32 planes carry no launch scale)
        const unsigned* cand = nullptr;
        int n_cand = 0;
        const float* g = g_raw[j];
        int rc = PLNERF_OK;
        if (act) {      // one pass, first: the activation's derivative (every kernel below reads the effective gradient) and the launch scale's maximum
            float* g_eff = (float*)(ws + lo.g_eff);
            rc = impl::absmax_act(g, raw_out[j], density_beta, n_rows[j], g_eff, gmax, st);
            g = g_eff;
        } else if (half && g_absmax && g_absmax[j] && n_absmax && n_absmax[j] > 0) {
            // the caller's producer kernel left the candidates (plnerf_quad_bwd's absmax_out): no pass, no memset -- the
            // gradient chain's workgroups take their maximum and leave it in the workspace's word for the kernels behind
            cand = g_absmax[j];
            n_cand = n_absmax[j];
        } else if (half) {
            rc = impl::absmax(g, (size_t)n_rows[j] * 4, gmax, st);
        }
        if (rc) return rc;
        wj[j] = impl::WgradJob{g, n_rows[j], saved[j], ws + lo.dz, gmax, (float*)(ws + lo.partials), (float*)(ws + lo.head_part),
                               grads + j * PLNERF_N_PARAM_TENSORS, input_ch, input_ch_views, saved_layout[j],
                               status_word(const_cast<void*>(packed[j]), precision), status_out ? status_out[j] : nullptr,
                               half ? compose_block(packed[j], precision) : nullptr, half ? (float*)(ws + lo.gred) : nullptr,
                               compact ? 1 : 0};
        if (half) {
            dj[j] = impl::DgradJob{packed[j], ns_of(precision), g, n_rows[j], saved[j], ws + lo.dz, gmax, cand, n_cand,
                                   compact ? (const unsigned*)(ws + lo.partials) : nullptr};
            if (compact) lj[n_live_jobs++] = impl::LiveJob{g, n_rows[j], (float*)(ws + lo.partials)};
        } else {
            rc = impl::f32_dgrad(packed[j], g, n_rows[j], (const float*)saved[j], (float*)(ws + lo.dz), st);
            if (!rc) rc = impl::wgrad_f32(wj[j], st);
            if (rc) return rc;
        }
    }
    if (!half) return PLNERF_OK;
    int rc = n_live_jobs ? impl::live_list(n_live_jobs, lj, st) : PLNERF_OK;      // (on this stream, ahead of dgrad; the host reads nothing back)
    if (rc) return rc;
    rc = impl::h16_dgrad(n_jobs, dj, st);
    if (rc) return rc;
    return impl::wgrad_h16_multi(n_jobs, wj, st);
}

extern "C" int plnerf_mlp_bwd(const void* packed, int precision, const float* g_raw, const uint32_t* g_absmax, int n_absmax,
                              int input_ch, int input_ch_views, int n_rows, const void* saved, int saved_layout,
                              const float* raw_out, float density_beta, void* workspace,
                              float* const* grads, float* status_out, plnerf_stream_t stream) {
    if (!grads) return PLNERF_EINVAL;
    return plnerf_mlp_bwd_multi(1, &packed, precision, &g_raw, &g_absmax, &n_absmax, input_ch, input_ch_views, &n_rows, &saved,
                                &saved_layout, &raw_out, density_beta, &workspace, grads, &status_out, stream);
}

extern "C" int plnerf_mlp_input_grad(const float* const* params, int precision, int input_ch, int input_ch_views,
                                     int n_rows, const void* workspace, float* g_embedded, plnerf_stream_t stream) {
    if (!known(precision)) return PLNERF_ENOSYS;
    if (!params || !workspace || !g_embedded || n_rows < 1 || !geometry_ok(input_ch, input_ch_views)) return PLNERF_EINVAL;
    for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
        if (!params[i]) return PLNERF_EINVAL;
    if (precision == PLNERF_PREC_FP32)
        return impl::input_grad(params, n_rows, workspace, nullptr, false, input_ch, input_ch_views, g_embedded, nullptr, (hipStream_t)stream);
    const unsigned char* ws = (const unsigned char*)workspace;      // the dz planes and the launch scale's word, where plnerf_mlp_bwd left them
    const bwdplan::Workspace lo = bwdplan::workspace((size_t)n_rows, true);
    // (a backward over the live rows left compact planes and the list: the same decision as plnerf_mlp_bwd_multi's, on the same n_rows
    // -- of a one-network call, or of a merged one whose every network had room for its list, i.e. any that fits the device)
    const unsigned* live = impl::bwd_compact(n_rows) ? (const unsigned*)(ws + lo.partials) : nullptr;
    return impl::input_grad(params, n_rows, ws + lo.dz, (const unsigned*)(ws + lo.gmax), true, input_ch, input_ch_views, g_embedded,
                            live, (hipStream_t)stream);
}

// ---- include/experimental/plnerf_hip_unique.h: the fine pass's forward over the rows it needs (mlp_unique_plan.h) ----
static_assert(sizeof(plnerf_unique_layout) == 10 * sizeof(size_t), "");

extern "C" size_t plnerf_mlp_unique_workspace_bytes(int n_rows) { return n_rows < 1 ? 0 : uniq::workspace((size_t)n_rows).total; }

extern "C" int plnerf_mlp_unique_layout(int n_rows, plnerf_unique_layout* layout) {
    if (!layout || n_rows < 1) return PLNERF_EINVAL;
    const uniq::Workspace w = uniq::workspace((size_t)n_rows);
    *layout = plnerf_unique_layout{w.words, w.rows_u, w.src, w.pts_u, w.dirs_u, w.raw_u, w.g_raw_u, w.absmax,
                                   (size_t)uniq::blocks((size_t)n_rows), w.total};
    return PLNERF_OK;
}

extern "C" int plnerf_mlp_fwd_unique_served(int precision, int has_embedded, int fwd_kernel, int samples_per_ray, int n_rows,
                                            int training) {
    if (!known(precision) || !ns_of(precision) || !kernel_arg_ok(fwd_kernel) || n_rows < 1 || samples_per_ray < 1) return 0;
    return uniq::served(elem_of(precision), ns_of(precision), training != 0, has_embedded != 0, fwd_kernel, samples_per_ray,
                        (size_t)n_rows, impl::bwd_compact(n_rows), impl::fwd_unique_enabled()) ? 1 : 0;
}

extern "C" int plnerf_mlp_fwd_unique(const void* packed, int precision, const float* pts, const float* viewdirs, int input_ch,
                                     int input_ch_views, int n_rows, int samples_per_ray, float input_scale, float density_beta,
                                     float* raw_out, void* saved, int fwd_kernel, void* workspace, plnerf_stream_t stream) {
    if (!known(precision)) return PLNERF_ENOSYS;
    if (!kernel_arg_ok(fwd_kernel)) return PLNERF_EINVAL;
    if (n_rows < 0 || !geometry_ok(input_ch, input_ch_views) || !(density_beta >= 0.0f) || !(density_beta < 1e6f)) return PLNERF_EINVAL;
    if ((input_ch - 3) % 6 != 0 || input_ch < 3 || input_ch > lay::XYZ_CH || (input_ch_views - 3) % 6 != 0 || input_ch_views < 3 ||
        input_ch_views > lay::DIR_CH || !(input_scale > 0.0f) || !(input_scale < 1e6f))
        return PLNERF_EINVAL;
    if (n_rows == 0) return PLNERF_OK;
    if (!packed || !raw_out || !aligned16(raw_out) || !pts || !viewdirs || samples_per_ray < 1) return PLNERF_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 255) != 0) return PLNERF_EINVAL;
    if (!plnerf_mlp_fwd_unique_served(precision, 0, fwd_kernel, samples_per_ray, n_rows, saved != nullptr)) return PLNERF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const uniq::Workspace lo = uniq::workspace((size_t)n_rows);
    unsigned char* ws = (unsigned char*)workspace;
    int rc = impl::unique_list(pts, viewdirs, n_rows, samples_per_ray, workspace, st);
    if (rc) return rc;
    // the forward over the compact rows: one direction per row, the grid and the planes' stride from n_rows, the row count
    // from the device (a workgroup past it returns at once)
    rc = impl::rr_fwd(elem_of(precision), packed, (const unsigned char*)packed + impl::h16_packed_bytes(ns_of(precision)),
                      ns_of(precision), (const float*)(ws + lo.pts_u), (const float*)(ws + lo.dirs_u), nullptr, input_ch,
                      input_ch_views, n_rows, 1, impl::FwdOpt{input_scale, density_beta}, (float*)(ws + lo.raw_u), saved,
                      status_word(const_cast<void*>(packed), precision), st, (const unsigned*)(ws + lo.words));
    if (rc) return rc;
    return impl::unique_expand(n_rows, workspace, raw_out, st);
}

extern "C" int plnerf_mlp_unique_fold(const float* g_raw, int n_rows, void* workspace, plnerf_stream_t stream) {
    if (n_rows < 1 || !g_raw || !aligned16(g_raw) || !workspace || ((uintptr_t)workspace & 255) != 0) return PLNERF_EINVAL;
    return impl::unique_fold(g_raw, n_rows, workspace, (hipStream_t)stream);
}

bool plnerf::impl::fwd_unique_enabled() {
    const char* e = getenv("PLNERF_FWD_UNIQUE");
    return !(e && e[0] == '0' && e[1] == '\0');
}

// PLNERF_BWD_COMPACT=0: the dense backward (A/B measurements, the tests' dense leg).  Read at every call, so a process may
// switch between two backwards -- not between a backward and the plnerf_mlp_input_grad that reads its workspace.
bool plnerf::impl::bwd_compact(int n_rows) {
    if (n_rows < 1 || !bwdplan::live_list_fits((size_t)n_rows)) return false;
    const char* e = getenv("PLNERF_BWD_COMPACT");
    return !(e && e[0] == '0' && e[1] == '\0');
}
