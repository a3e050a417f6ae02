// Which forward kernel a 16-bit-mode call runs on: the register-resident kernel (mlp_rr_body.inc) or the ping-pong
// kernel (mlp_h16_fwd_pp.inc).  Plain C++ -- no HIP include -- so that a host compiler can build it
// (tests/test_mlp_fwd_route.py).
//
// PLNERF_RR_INSTANCES is THE list of register-resident instantiations, rows of (element, NS, SAVE, EMB):
//   element  f16 | bf16: IEEE-half or bf16 operands (namespaces plnerf_rr | plnerf_rr_bf16)
//   NS       1: plain operands; 2: 3-term split
//   SAVE     the training forward (writes the saved planes, in lay::SV_LAYOUT_TILED)
//   EMB      reads a caller-embedded input instead of encoding pts / viewdirs itself
// The declarations and the dispatch of mlp_rr.hip and rr_exists() below expand it; csrc/Makefile's RR_INST names the
// same rows, one object each (mlp_rr_inst.hip).  To add a variant: a row here and its stem there.  A row without its
// stem fails the library's link (an undefined launcher), a stem without its row fails to compile (mlp_rr_inst.hip),
// and tests/test_mlp_fwd_route.py compares the two lists.
#pragma once

#define PLNERF_RR_INSTANCES_f16(X) \
    X(f16, 1, 0, 0) X(f16, 1, 1, 0) X(f16, 2, 0, 0) X(f16, 2, 1, 0) X(f16, 2, 0, 1) X(f16, 2, 1, 1)
// (plain bf16 has no training variant, neither plain mode an embedded one)
#define PLNERF_RR_INSTANCES_bf16(X) \
    X(bf16, 1, 0, 0) X(bf16, 2, 0, 0) X(bf16, 2, 1, 0) X(bf16, 2, 0, 1) X(bf16, 2, 1, 1)
#define PLNERF_RR_INSTANCES(X) PLNERF_RR_INSTANCES_f16(X) PLNERF_RR_INSTANCES_bf16(X)
// The COUNTED variants of rows above (a device-side row count, RrFwdArgs::n_dev: the unique-row forward of the split modes,
// mlp_unique_plan.h), rows of (element, NS, SAVE); EMB is 0.  A list of its own, expanded by mlp_rr.hip and named again by
// csrc/Makefile's RR_CNT_INST (objects mlp_rr_c_<element>_<NS>_<SAVE>.o from mlp_rr_inst.hip with -DRR_INST_CNT); the plain
// rows and their objects are what they were.
#define PLNERF_RR_CNT_INSTANCES_f16(X) X(f16, 2, 0) X(f16, 2, 1)
#define PLNERF_RR_CNT_INSTANCES_bf16(X) X(bf16, 2, 0) X(bf16, 2, 1)
#define PLNERF_RR_CNT_INSTANCES(X) PLNERF_RR_CNT_INSTANCES_f16(X) PLNERF_RR_CNT_INSTANCES_bf16(X)
#define PLNERF_RR_CNT_LAUNCHER_(E, NS, SAVE) rr_launch_cnt_##E##_##NS##_##SAVE
#define PLNERF_RR_CNT_LAUNCHER(E, NS, SAVE) PLNERF_RR_CNT_LAUNCHER_(E, NS, SAVE)
// the launcher behind a row: int rr_launch_<element>_<NS>_<SAVE>_<EMB>(const RrFwdArgs&, hipStream_t)
#define PLNERF_RR_LAUNCHER_(E, NS, SAVE, EMB) rr_launch_##E##_##NS##_##SAVE##_##EMB
#define PLNERF_RR_LAUNCHER(E, NS, SAVE, EMB) PLNERF_RR_LAUNCHER_(E, NS, SAVE, EMB)
// the element of a translation unit that includes mlp_rr_body.inc (compiled with -DRR_BF16 or without), for names that
// carry it: PLNERF_RR_PASTE(rr_pack_, PLNERF_RR_ELEM)
#ifdef RR_BF16
#define PLNERF_RR_ELEM bf16
#else
#define PLNERF_RR_ELEM f16
#endif
#define PLNERF_RR_PASTE_(a, b) a##b
#define PLNERF_RR_PASTE(a, b) PLNERF_RR_PASTE_(a, b)

namespace plnerf {
namespace route {

enum { ELEM_f16 = 0, ELEM_bf16 = 1 };
enum { FWD_AUTO = 0, FWD_RR = 1, FWD_PP = 2 };      // = PLNERF_FWD_KERNEL_* (plnerf_hip.h; mlp_api.hip asserts it)

constexpr bool rr_exists(int elem, int ns, bool save, bool emb) {
#define PLNERF_RR_ROW(E, NS, SAVE, EMB) (elem == ELEM_##E && ns == NS && save == bool(SAVE) && emb == bool(EMB)) ||
    return PLNERF_RR_INSTANCES(PLNERF_RR_ROW) false;
#undef PLNERF_RR_ROW
}

// true: the register-resident kernel.  `forced` (the ABI's fwd_kernel argument) selects a kernel wherever it exists:
// A/B measurements and the test suite's other passes.  AUTO, measured: the split modes run on the register-resident
// kernel throughout -- inference +20 % over the ping-pong kernel, the training forward -15 % per launch -- and so does
// plain inference (two row tiles per wave: +18 %); the plain training forward keeps the ping-pong kernel (its 5.3 KB of
// plane stores per row come out of eight waves per CU there, out of four here: 1.22 vs 1.39 ms).
constexpr bool fwd_uses_rr(int elem, int ns, bool training, bool embedded, int forced) {
    if (forced == FWD_PP || !rr_exists(elem, ns, training, embedded)) return false;
    return forced == FWD_RR || ns == 2 || !training;
}

}  // namespace route
}  // namespace plnerf
