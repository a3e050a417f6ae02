// The host-side description of a network of the layer-by-layer route, shared by its one-call entries: the no-grad forward
// (linear_h16_chain.hip, include/experimental/plnerf_hip_generic.h) and the training forward and backward
// (linear_h16_chain.hip, linear_h16_bwd.hip, include/experimental/plnerf_hip_generic_train.h).
//   Net, describe     the layers in state_dict order, their sizes, the refusals of a shape
//   weight_offset     where a layer's packed weights lie (both forwards put them first)
//   TrainLayout       where everything else lies in the training entries' `saved` state and in the backward's workspace
//   wgrad_splits      the k_splits of a weight gradient
// Internal: every including file gets its own copies.
#pragma once

#include <vector>

#include "linear_h16_dev.h"
#include "../../include/experimental/plnerf_hip_generic.h"

namespace {

constexpr int MAX_DIM = 65536;            // of every size of the shape (keeps the byte counts far inside size_t)
constexpr size_t WS_ALIGN = 256;          // of every piece inside a workspace or a saved state

inline size_t round_up(const size_t v, const size_t to) { return (v + to - 1) / to * to; }

struct Net {
    const plnerf_generic_shape* s;
    int views, width_out;                 // view layers that run; columns of the output
    int n_layers;                         // in state_dict order: D trunk, n_view_layers view, then feature / alpha / rgb or output
    bool skip(const int i) const {
        for (int q = 0; q < s->n_skips; ++q)
            if (s->skips[q] == i) return true;
        return false;
    }
    int feature() const { return s->D + s->n_view_layers; }      // (also output_linear's slot)
    bool runs(const int l) const { return s->use_viewdirs || l < s->D || l >= feature(); }
    void dims(const int l, int& N, int& K) const {
        const int D = s->D, W = s->W;
        if (l < D) {
            N = W;
            K = l == 0 ? s->input_ch : skip(l - 1) ? s->input_ch + W : W;
        } else if (l < feature()) {
            N = W / 2;
            K = l == D ? W + s->view_ch : W / 2;
        } else if (!s->use_viewdirs) {
            N = s->output_ch;
            K = W;
        } else if (l == feature()) {
            N = W;
            K = W;
        } else if (l == feature() + 1) {
            N = 1;
            K = W;
        } else {
            N = 3;
            K = W / 2;
        }
    }
};

// PLNERF_OK and the network's description, or the refusal
inline int describe(const plnerf_generic_shape* s, const int precision, Net& net) {
    if (!s || !is_h16(precision)) return PLNERF_EINVAL;
    if (s->D < 1 || s->W < 1 || s->input_ch < 1 || s->view_ch < 0 || s->n_view_layers < 0 || s->n_skips < 0 ||
        s->n_skips > PLNERF_GENERIC_MAX_SKIPS)
        return PLNERF_EINVAL;
    if (s->use_viewdirs ? (s->W < 2 || s->n_view_layers < 1) : s->output_ch < 1) return PLNERF_EINVAL;
    for (int q = 0; q < s->n_skips; ++q)
        if (s->skips[q] < 0 || s->skips[q] > s->D - 2) return PLNERF_EINVAL;
    if (s->D > MAX_DIM || s->W > MAX_DIM || s->input_ch > MAX_DIM || s->view_ch > MAX_DIM || s->n_view_layers > MAX_DIM ||
        (!s->use_viewdirs && s->output_ch > MAX_DIM))
        return PLNERF_ERANGE;
    net.s = s;
    net.views = s->use_viewdirs ? s->n_view_layers : 0;
    net.width_out = s->use_viewdirs ? 4 : s->output_ch;
    net.n_layers = s->D + s->n_view_layers + (s->use_viewdirs ? 3 : 1);
    return PLNERF_OK;
}

// byte offset of layer l's packed weights (layers that do not run take no room)
inline size_t weight_offset(const Net& net, const int l, const int planes) {
    size_t off = 0;
    for (int q = 0; q < l; ++q) {
        if (!net.runs(q)) continue;
        int N, K;
        net.dims(q, N, K);
        off += round_up(PLNERF_PACK_BYTES(N, K, planes), WS_ALIGN);
    }
    return off;
}

// every launch's grid, before the first: the widest layer's tiles, the copies' workgroups
inline int check_grids(const Net& net, const int n, const bool copies) {
    const plnerf_generic_shape* s = net.s;
    const int widest = s->use_viewdirs || s->W > s->output_ch ? s->W : s->output_ch;
    if ((((long long)n + 127) / 128) * (((long long)widest + 127) / 128) > 0x7fffffffLL) return PLNERF_ERANGE;
    const int widest_copy = s->input_ch > s->view_ch ? s->input_ch : s->view_ch;
    if (copies && ((long long)n * widest_copy + THREADS - 1) / THREADS > 0x7fffffffLL) return PLNERF_ERANGE;
    return PLNERF_OK;
}

// ---- the training entries
// k_splits of the weight gradient [N, K1] over M rows: generic._splits, restated
inline int wgrad_splits(const int N, const int K1, const int M) {
    const long long tiles = (((long long)N + 63) / 64) * (((long long)K1 + 63) / 64);
    if (tiles <= 0 || tiles >= 256) return 1;
    const long long by_tiles = 1024 / tiles, by_rows = M / 512, s = by_tiles < by_rows ? by_tiles : by_rows;
    return s > 1 ? (int)s : 1;
}

inline long long gate_ld(const int N) { return ((long long)N + 31) / 32; }      // words per row of a gate plane

// `saved`: the packed weights; then per layer, in layer order, what its forward leaves -- a ReLU layer's gate plane
// [n, gate_ld(N)] words, and its output: packed [n, N], or, where a concatenation follows (a skip; feature_linear), the fp32
// rows [n, ld_cat] of that concatenation, the layer's columns behind the encoding's (before the view columns).  NONE: nothing.
// The backward's workspace: one max-|g| word per layer, two fp32 gradient buffers [n, ld_g], the weight gradient's partials.
struct TrainLayout {
    static constexpr size_t NONE = ~(size_t)0;
    std::vector<size_t> act, gate, cat, weight;
    long long ld_cat_trunk, ld_cat_view;      // floats per concatenation row (multiples of four)
    size_t saved_bytes;
    size_t words, g[2], partials, workspace_bytes;
    long long ld_g;
};

inline bool relu_layer(const Net& net, const int l) { return l < net.feature(); }

inline TrainLayout lay_out_train(const Net& net, const int n, const int planes) {
    const plnerf_generic_shape* s = net.s;
    TrainLayout t;
    t.act.assign(net.n_layers, TrainLayout::NONE);
    t.gate = t.cat = t.weight = t.act;
    t.ld_cat_trunk = ((long long)s->input_ch + s->W + 3) / 4 * 4;
    t.ld_cat_view = ((long long)s->W + s->view_ch + 3) / 4 * 4;
    size_t off = 0, partials = 0;
    for (int l = 0; l < net.n_layers; ++l) {
        if (!net.runs(l)) continue;
        int N, K;
        net.dims(l, N, K);
        t.weight[l] = off;
        off += round_up(PLNERF_PACK_BYTES(N, K, planes), WS_ALIGN);
        const int splits = wgrad_splits(N, K + 1, n);
        const size_t need = splits > 1 ? (size_t)splits * (size_t)N * ((size_t)K + 1) * sizeof(float) : 0;
        partials = need > partials ? need : partials;
    }
    for (int l = 0; l < net.n_layers; ++l) {
        if (!net.runs(l)) continue;
        int N, K;
        net.dims(l, N, K);
        if (relu_layer(net, l)) {
            t.gate[l] = off;
            off += round_up((size_t)n * (size_t)gate_ld(N) * sizeof(unsigned), WS_ALIGN);
        }
        if (l < s->D && net.skip(l)) {
            t.cat[l] = off;
            off += round_up((size_t)n * (size_t)t.ld_cat_trunk * sizeof(float), WS_ALIGN);
        } else if (s->use_viewdirs && l == net.feature()) {
            t.cat[l] = off;
            off += round_up((size_t)n * (size_t)t.ld_cat_view * sizeof(float), WS_ALIGN);
        } else if (relu_layer(net, l)) {
            t.act[l] = off;
            off += round_up(PLNERF_PACK_BYTES(n, N, planes), WS_ALIGN);
        }
    }
    t.saved_bytes = off;
    t.ld_g = ((long long)s->W + 3) / 4 * 4;
    const size_t g_bytes = round_up((size_t)n * (size_t)t.ld_g * sizeof(float), WS_ALIGN);
    t.words = 0;
    t.g[0] = round_up((size_t)net.n_layers * sizeof(unsigned), WS_ALIGN);
    t.g[1] = t.g[0] + g_bytes;
    t.partials = t.g[1] + g_bytes;
    t.workspace_bytes = t.partials + round_up(partials, WS_ALIGN);
    return t;
}

}  // namespace
