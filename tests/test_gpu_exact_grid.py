"""The MLP kernels bit for bit on an exactly representable network (tests/exact_grid_cases.py: sparse +-1 weights, integer
rows and cotangents, ~30 % of the rows with a zero cotangent, a whole dead tile among them; tests/test_exact_grid_host.py checks
its conditions on the CPU).  Every input, weight, activation and scaled pre-activation gradient is an integer that fits the
narrowest 16-bit format in use and every sum stays below 2^24, so every conversion, every fp32 MFMA chain, every split-K order
and the power-of-two launch scale are exact: the GPU result must EQUAL the float64 reference in every entry, in all five
precisions and on both forward kernels.  A mismatch is a wrong index, gate, scale, tile edge or compaction, never rounding --
there is no tolerance in this file.

The raw ABI as tests/test_gpu_grad_range.py uses it, with the caller-supplied encoding (`embedded`), at 1, 33, 64, 65, 193, 257
and 1000 rows; workspace (one 0.3 GB buffer for all cases) and outputs poisoned with NaN before each call.  Comparisons are on
the bit patterns against the float32 cast of the reference, -0 taken as 0.

  1. test_training_forward       plnerf_mlp_fwd with a saved state: raw_out.
  2. test_inference_forward      saved == NULL, kernels AUTO, RR and PP: the same raw_out.
  3. test_backward               plnerf_mlp_bwd + plnerf_mlp_input_grad: the 24 gradients and g_embedded, by the call's own pass
                                 over g_raw; test_backward_with_g_absmax once per variant with the maximum handed in.
  4. test_scaled_cotangent       g_raw 2^-40 and 2^40 at 257 rows: the reference scaled by the same power.
  5. test_two_jobs               plnerf_mlp_bwd_multi on two seeds' networks (193 and 65 rows); again with the second job's g_raw
                                 all zero: its gradients exactly zero, the first job's unchanged.
  6. test_python_mirror          make_net(...)(embedded), backward: the same bits.
  7. the network's range status word is 0 after every one of them.

What this file cannot see: the rounding modes of conversions (nothing here rounds), the lo planes of the x3 forward (they are
zero), the accumulation order (every order gives the same integers), the in-kernel encoding and the density activation."""
import ctypes

import numpy as np
import pytest
import torch

import exact_grid_cases as C
from grad_range_cases import absmax_candidates      # (max |g_raw| as plnerf_quad_bwd's absmax_out hands it over)
from gpu_support import P, dev, g, make_net  # noqa: F401

pytestmark = pytest.mark.gpu

KERNELS = {"auto": 0, "rr": 1, "pp": 2}      # PLNERF_FWD_KERNEL_*
MODES = ("fp32", "f16x3", "bf16x3", "f16", "bf16")
# tests/test_gpu_grad_range.py's VARIANTS, restated: every training variant of the 16-bit modes (there is no register-resident
# training forward in plain bf16), and the exact-fp32 kernels
VARIANTS = [("fp32", "auto")] + [(mode, kernel) for mode in MODES[1:] for kernel in ("rr", "pp") if (mode, kernel) != ("bf16", "rr")]
ids = lambda v: "-".join(v)
XC, DC = C.XC, C.DC
_STATES, _WORKSPACES = {}, {}


def workspace(L, n, prec, slot=0):
    """The first words of one buffer as large as any case here needs (slot 1: the second job's of test_two_jobs)."""
    if slot not in _WORKSPACES:
        words = max(L.lib().plnerf_mlp_bwd_workspace_bytes(m, L.PRECISION[mode]) for m in C.ROWS for mode in MODES) // 4
        _WORKSPACES[slot] = torch.empty(words, device=dev())
    words = L.lib().plnerf_mlp_bwd_workspace_bytes(n, prec) // 4
    assert 0 < words <= _WORKSPACES[slot].numel()
    return _WORKSPACES[slot][:words]


def poisoned(*shape):
    return torch.full(shape, float("nan"), device=dev())


class State:
    """One (variant, rows, seed): the network, packed, and its training forward."""

    def __init__(self, P, mode, kernel, n, seed):
        from plnerf_amd import _lib as L
        self.L, self.mode, self.kernel, self.prec, self.n = L, mode, kernel, L.PRECISION[mode], n
        self.case = C.build(n, seed)
        self.net = make_net(P, self.case.sd, mode)
        self.packed = self.net.packed_weights()
        self.params = list(self.net.parameters())
        assert [name for name, _ in self.net.named_parameters()] == self.case.names
        self.layout = L.lib().plnerf_mlp_saved_layout(self.prec, 1, KERNELS[kernel])
        self.emb = g(torch.from_numpy(np.array(self.case.embedded)))
        self.saved = poisoned(L.lib().plnerf_mlp_saved_bytes(n, self.prec) // 4)
        self.raw = self.forward(kernel, self.saved)

    def forward(self, kernel, saved=None):
        L = self.L
        raw = poisoned(self.n, 4)
        L.check(L.lib().plnerf_mlp_fwd(L.dptr(self.packed), self.prec, None, None, L.dptr(self.emb), XC, DC, self.n, 1, 1.0, 0.0,
                                       L.dptr(raw), L.dptr(saved), KERNELS[kernel], L.stream()), "plnerf_mlp_fwd")
        torch.cuda.synchronize()
        return raw.cpu().numpy()

    def grad_buffers(self):
        return [poisoned(*p.shape) for p in self.params], poisoned(self.n, XC + DC)

    def backward(self, g_raw, with_absmax=False):
        """plnerf_mlp_bwd, then plnerf_mlp_input_grad on its workspace: the 24 parameter gradients and g_embedded, as numpy."""
        L = self.L
        assert g_raw.dtype == np.float32 and g_raw.shape == (self.n, 4)
        ws = workspace(L, self.n, self.prec)
        ws.fill_(float("nan"))
        grads, g_emb = self.grad_buffers()
        g_dev = g(torch.from_numpy(np.array(g_raw)))
        cand = g(torch.from_numpy(absmax_candidates(g_raw))) if with_absmax else None
        L.check(L.lib().plnerf_mlp_bwd(L.dptr(self.packed), self.prec, L.dptr(g_dev), L.dptr(cand, "g_absmax", torch.int32),
                                       0 if cand is None else cand.numel(), XC, DC, self.n, L.dptr(self.saved), self.layout, None, 0.0,
                                       L.dptr(ws), L.ptr_table(grads, "grads"), None, L.stream()), "plnerf_mlp_bwd")
        L.check(L.lib().plnerf_mlp_input_grad(L.ptr_table(self.params, "params"), self.prec, XC, DC, self.n, L.dptr(ws),
                                              L.dptr(g_emb), L.stream()), "plnerf_mlp_input_grad")
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in grads + [g_emb]]

    def status(self):
        return self.net.range_status()


def state_of(P, variant, n, seed=C.SEED):
    key = (variant, n, seed)
    if key not in _STATES:
        _STATES[key] = State(P, *variant, n, seed)
    return _STATES[key]


def mismatches(names, got, want):
    """[(tensor, entries that differ, first index, got there, wanted there)] on the bit patterns, -0 taken as 0."""
    out = []
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, name
        a, b = np.where(a == 0, np.float32(0), a), np.where(b == 0, np.float32(0), b)
        bad = np.ascontiguousarray(a).view(np.int32) != np.ascontiguousarray(b).view(np.int32)
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            out.append((name, int(bad.sum()), at, float(a[at]), float(b[at])))
    return out


def reference(case, k=0):
    return [np.ldexp(a, k) for a in case.grads + [case.g_embedded]]


# ----------------------------------------------------------------------------- 1, 2: the forwards
@pytest.mark.parametrize("n", C.ROWS)
@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_training_forward(P, variant, n):
    st = state_of(P, variant, n)
    assert not mismatches(["raw"], [st.raw], [st.case.raw])
    assert st.status() == 0


@pytest.mark.parametrize("n", C.ROWS)
@pytest.mark.parametrize("mode", MODES)
def test_inference_forward(P, mode, n):
    """saved == NULL.  AUTO, RR and PP: a forced kernel runs wherever that variant exists, the product's choice otherwise."""
    st = state_of(P, (mode, "auto" if mode == "fp32" else "pp"), n)
    bad = [(kernel, mismatches(["raw"], [st.forward(kernel)], [st.case.raw])) for kernel in KERNELS]
    assert not [b for b in bad if b[1]], bad
    assert st.status() == 0


# ----------------------------------------------------------------------------- 3: the backward
@pytest.mark.parametrize("n", C.ROWS)
@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_backward(P, variant, n):
    """All 24 gradients and g_embedded, the launch scale from the call's own pass over g_raw.  The rows with a zero cotangent
    (the dead tile, the tile whose only live row is its last) leave exact zeros in g_embedded and add nothing."""
    st = state_of(P, variant, n)
    assert not mismatches(st.case.names + ["g_embedded"], st.backward(st.case.g_raw), reference(st.case))
    assert st.status() == 0


@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_backward_with_g_absmax(P, variant):
    """The same with max |g_raw| handed in (g_absmax): the gradient chain's workgroups take the maximum themselves."""
    st = state_of(P, variant, 1000)
    assert not mismatches(st.case.names + ["g_embedded"], st.backward(st.case.g_raw, with_absmax=True), reference(st.case))
    assert st.status() == 0


# ----------------------------------------------------------------------------- 4: the scaled cotangent
@pytest.mark.parametrize("k", (-40, 40))
@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_scaled_cotangent(P, variant, k):
    """g_raw 2^k: the launch scale moves by 2^-k, the planes hold the same integers, the un-scale is an exact power of two."""
    st = state_of(P, variant, 257)
    got = st.backward(np.ldexp(st.case.g_raw, k))
    assert not mismatches(st.case.names + ["g_embedded"], got, reference(st.case, k))
    assert st.status() == 0


# ----------------------------------------------------------------------------- 5: two jobs
@pytest.mark.parametrize("mode", MODES[1:])
def test_two_jobs(P, mode):
    """plnerf_mlp_bwd_multi on two seeds' networks, 193 and 65 rows: both exact.  Then the second job's g_raw all zero: no row
    of it is live, its 24 gradients are exactly zero, and the first job's are what they were."""
    from plnerf_amd import _lib as L
    jobs = [state_of(P, (mode, "auto"), n, seed) for n, seed in C.TWO_JOBS]
    prec = jobs[0].prec
    vp = lambda items: (ctypes.c_void_p * len(items))(*[None if x is None else x.value for x in items])
    for second_is_zero in (False, True):
        g_raws = [np.array(st.case.g_raw) for st in jobs]
        want = [st.case.grads for st in jobs]
        if second_is_zero:
            g_raws[1][:] = 0
            want = [want[0], [np.zeros_like(a) for a in want[1]]]
        ws = [workspace(L, st.n, prec, slot) for slot, st in enumerate(jobs)]
        for w in ws:
            w.fill_(float("nan"))
        grads = [st.grad_buffers()[0] for st in jobs]
        g_dev = [g(torch.from_numpy(a)) for a in g_raws]
        L.check(L.lib().plnerf_mlp_bwd_multi(
            2, vp([L.dptr(st.packed) for st in jobs]), prec, vp([L.dptr(t) for t in g_dev]), None, None, XC, DC,
            (ctypes.c_int * 2)(*[st.n for st in jobs]), vp([L.dptr(st.saved) for st in jobs]),
            (ctypes.c_int * 2)(*[st.layout for st in jobs]), None, 0.0, vp([L.dptr(w) for w in ws]),
            L.ptr_table([t for gr in grads for t in gr], "grads"), None, L.stream()), "plnerf_mlp_bwd_multi")
        torch.cuda.synchronize()
        for j, st in enumerate(jobs):
            bad = mismatches(st.case.names, [t.cpu().numpy() for t in grads[j]], want[j])
            assert not bad, (f"job {j}", "second job's g_raw zero" if second_is_zero else "both jobs live", bad)
    assert [st.status() for st in jobs] == [0, 0]


# ----------------------------------------------------------------------------- 6: the Python mirror
@pytest.mark.parametrize("mode", MODES)
def test_python_mirror(P, mode):
    """make_net(P, sd, mode), net(embedded), backward: autograd's route through functional.MlpFn gives the same bits."""
    case = C.build(65, C.SEED)
    net = make_net(P, case.sd, mode)
    emb = g(torch.from_numpy(np.array(case.embedded))).requires_grad_(True)
    raw = net(emb)
    raw.backward(g(torch.from_numpy(np.array(case.g_raw))))
    torch.cuda.synchronize()
    got = [raw.detach().cpu().numpy()] + [p.grad.cpu().numpy() for p in net.parameters()] + [emb.grad.cpu().numpy()]
    assert not mismatches(["raw"] + case.names + ["g_embedded"], got, [case.raw] + reference(case))
    assert net.range_status() == 0
