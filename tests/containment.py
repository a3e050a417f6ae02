"""The table behind tests/test_gpu_containment.py: every entry point of the C ABI that touches device memory, described
once -- its arguments in header order, each pointer's role, dtype, size as a function of the case's shape and the alignment
the header demands -- and the generic runner that calls such a description through the raw ABI on buffers carved out of a
sentinel arena (tests/arena.py).

A CASE is a list of Calls on named buffers (a Buf is a description; memory exists only while a run lasts).  A buffer that
one call writes may be an input of the next, so an entry that needs the results of another (a backward its forward's
indices, plnerf_mlp_input_grad the backward's workspace) is exercised on real data; the role is per call.  run_case()
carries a case out three times on identical inputs -- scratch at 0x00, scratch at 0xFF, and on ordinary torch allocations --
and holds the results to the conditions of the module docstring of tests/test_gpu_containment.py.

Nothing here needs a GPU to be BUILT: tests/test_containment_table.py builds every case on the CPU, checks each call
against the header's prototype (arity, pointer or scalar, const or not) and requires every declared entry to be in a case
or in EXEMPT.
"""
import ctypes
import math
import zlib

import torch

from arena import Arena, FILL, fill_words
from plnerf_amd import _lib

DTYPES = {"f32": (torch.float32, 4), "f64": (torch.float64, 8), "i32": (torch.int32, 4), "u32": (torch.int32, 4),
          "i64": (torch.int64, 8), "u8": (torch.uint8, 1), "u16": (torch.int16, 2)}
ROLES = ("in", "out", "scratch", "zeroed", "inout", "zero_once")
# zero_once: a one-call entry's workspace ("the caller ZEROES it once before the first step"): what must be zero is the loss
# kernel's block at its start (Buf.stays_zero), zero again after every step; the rest is scratch -- the arena runs fill it
# with 0x00 and 0xFF, the run on ordinary allocations zeroes all of it as the header says

# Entries outside the table, each with its reason.  Two reasons are acceptable: the entry writes no device memory, or it
# already has a sentinel test, which is named.
NO_DEVICE_WRITES = "writes no device memory"
EXEMPT = {
    "plnerf_version": NO_DEVICE_WRITES,
    "plnerf_build_flags": NO_DEVICE_WRITES,
    "plnerf_error_string": NO_DEVICE_WRITES,
    "plnerf_mlp_packed_bytes": NO_DEVICE_WRITES,
    "plnerf_mlp_status_offset": NO_DEVICE_WRITES,
    "plnerf_mlp_saved_bytes": NO_DEVICE_WRITES,
    "plnerf_mlp_bwd_workspace_bytes": NO_DEVICE_WRITES,
    "plnerf_mlp_saved_layout": NO_DEVICE_WRITES,
    "plnerf_sample_error_workspace_bytes": NO_DEVICE_WRITES,
    "plnerf_train_step_workspace_bytes": NO_DEVICE_WRITES,
    "plnerf_train_step_const_workspace_bytes": NO_DEVICE_WRITES,
    "plnerf_depth_train_step_workspace_bytes": NO_DEVICE_WRITES,
    "plnerf_depth_train_step_const_workspace_bytes": NO_DEVICE_WRITES,
    "plnerf_depth_train_step_layout": NO_DEVICE_WRITES,
    "plnerf_depth_train_step_const_layout": NO_DEVICE_WRITES,
    "plnerf_render_view_workspace_bytes": NO_DEVICE_WRITES,
    "plnerf_frame_export": "sentinel test: tests/test_gpu_view.py::test_frame_export_is_to8b_and_to16b "
                           "(through _export: not a byte before, none past 3 n / 2 n)",
}


# ---- descriptions ------------------------------------------------------------------------------------------------------
class Buf:
    """One device buffer of a case.  shape: element counts; data: the CPU tensor an `in` / `inout` buffer starts from;
    align: the header's demand (default: the element size); guard: the bytes one full tile of its widest writer covers
    (the arena never gives less than 64 KiB).
    pad: bool mask over the buffer's 4-byte words -- DOCUMENTED padding, which may hold anything (the fill included);
    untouched: bool mask over its words that no call may write (they must still hold the fill);
    opaque: the layout is private to the library (packed weights, saved activations of the 16-bit modes, workspaces): no
    word-level conditions, the buffer counts through the results computed from it;
    finite: fp results must be finite (the inputs always are); zero_at: (offset, bytes) zeroed by the caller after the
    fill (the packed buffer's status word); stays_zero: (offset, bytes) that must be zero after every call."""

    def __init__(self, name, dtype, shape, data=None, align=None, guard=0, pad=None, untouched=None, opaque=False,
                 finite=True, zero_at=None, stays_zero=None):
        self.name, self.dtype, self.shape = name, dtype, tuple(int(s) for s in shape)
        self.n = math.prod(self.shape)
        assert self.n > 0, (name, shape)
        self.nbytes = self.n * DTYPES[dtype][1]
        self.data, self.align, self.guard = data, int(align or DTYPES[dtype][1]), int(guard)
        self.pad, self.untouched, self.opaque, self.finite = pad, untouched, opaque, finite
        self.zero_at, self.stays_zero = zero_at, stays_zero
        if data is not None:
            assert data.dtype == DTYPES[dtype][0] and data.numel() == self.n, (name, data.dtype, tuple(data.shape), shape)


class Ref:
    """A buffer as one argument of one call: its role there, and a byte offset for a pointer into it."""

    def __init__(self, buf, role, offset=0):
        assert role in ROLES, role
        self.buf, self.role, self.offset = buf, role, int(offset)


def IN(buf, offset=0):
    return Ref(buf, "in", offset)


def OUT(buf, offset=0):
    return Ref(buf, "out", offset)


def INOUT(buf, offset=0):
    return Ref(buf, "inout", offset)


def SCRATCH(buf):
    return Ref(buf, "scratch")


def ZEROED(buf):
    return Ref(buf, "zeroed")


def ZERO_ONCE(buf):
    return Ref(buf, "zero_once")


class HostArray:
    """A typed array in HOST memory, read during the call (c2w_host, bb_center_host, the int tables of bwd_multi)."""

    def __init__(self, ctype, values):
        self.ctype, self.values = ctype, list(values)

    def make(self):
        return (self.ctype * len(self.values))(*self.values)


class PtrTable:
    """A host table of device pointers (params[24], grads[24], the per-job tables of plnerf_mlp_bwd_multi)."""

    def __init__(self, refs):
        self.refs = list(refs)      # Ref or None


class Struct:
    """A host struct of the one-call entries: build(addr) returns the ctypes instance, addr(ref) the device address of a
    Ref (None -> None).  refs: every Ref the struct points at."""

    def __init__(self, refs, build):
        self.refs, self.build = list(refs), build


class Call:
    def __init__(self, entry, *args):
        self.entry, self.args = entry, args      # (the stream is appended by the runner: every such entry ends with it)

    def refs(self):
        out = []
        for a in self.args:
            if isinstance(a, Ref):
                out.append(a)
            elif isinstance(a, PtrTable):
                out += [r for r in a.refs if r is not None]
            elif isinstance(a, Struct):
                out += [r for r in a.refs if r is not None]
        return out


# ---- deterministic data ------------------------------------------------------------------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def uniform(name, *shape, lo=0.0, hi=1.0):
    return Buf(name, "f32", shape, data=torch.rand(*shape, generator=_gen(name)) * (hi - lo) + lo)


def normal(name, *shape, scale=1.0, **kw):
    return Buf(name, "f32", shape, data=torch.randn(*shape, generator=_gen(name)) * scale, **kw)


def given(name, dtype, tensor, **kw):
    return Buf(name, dtype, tuple(tensor.shape) or (1,), data=tensor.contiguous().to(DTYPES[dtype][0]), **kw)


def out(name, dtype, *shape, **kw):
    return Buf(name, dtype, shape, **kw)


def sorted_depths(name, near, far, R, S):
    """[R,S] strictly inside (near, far), ascending per ray."""
    t = torch.sort(torch.rand(R, S, generator=_gen(name)) * 0.98 + 0.01, dim=1).values
    return given(name, "f32", near.data[:, None] + (far.data - near.data)[:, None] * t)


# ---- the runner --------------------------------------------------------------------------------------------------------
class _Plain:
    """A buffer of the third run: an ordinary torch allocation of its own."""

    def __init__(self, buf, device):
        self.mem = torch.empty(buf.nbytes, dtype=torch.uint8, device=device)
        self.snapshot = None

    def u8(self):
        return self.mem

    @property
    def dptr(self):
        return self.mem.data_ptr()

    def put(self, tensor):
        self.mem.copy_(tensor.contiguous().reshape(-1).view(torch.uint8))

    def set_bytes(self, byte):
        self.mem.fill_(byte)

    def freeze(self):
        self.snapshot = self.mem.clone()


def marshal(call, addr):
    """The ctypes arguments of one Call (without the stream): addr(ref) gives the address of a Ref, None of None.  Returns
    (arguments, objects to keep alive across the call)."""
    keep, cargs = [], []
    for a in call.args:
        if isinstance(a, Ref):
            cargs.append(ctypes.c_void_p(addr(a)))
        elif isinstance(a, PtrTable):
            keep.append((ctypes.c_void_p * len(a.refs))(*[addr(r) for r in a.refs]))
            cargs.append(keep[-1])
        elif isinstance(a, HostArray):
            keep.append(a.make())
            cargs.append(keep[-1])
        elif isinstance(a, Struct):
            keep.append(a.build(addr))
            cargs.append(ctypes.byref(keep[-1]))
        else:
            cargs.append(a)
    return cargs, keep


def case_buffers(calls):
    """{name: (Buf, role of its first appearance, every role)} in order of first appearance."""
    bufs = {}
    for c in calls:
        for r in c.refs():
            if r.buf.name in bufs:
                assert bufs[r.buf.name][0] is r.buf, f"two buffers named {r.buf.name}"
                bufs[r.buf.name][2].add(r.role)
            else:
                bufs[r.buf.name] = (r.buf, r.role, {r.role})
    return bufs


def _span_is_zero(handle, span):
    return not bool(handle.u8()[span[0]:span[0] + span[1]].any())


def run_once(L, calls, scratch_fill, device):
    """Carry the case out once.  scratch_fill 0x00 / 0xFF: every buffer carved from ONE arena, scratch at that byte;
    None: every buffer an ordinary allocation.  Returns {name: the final bytes (CPU)} of every buffer some call wrote."""
    bufs = case_buffers(calls)
    arena = None
    if scratch_fill is not None:
        arena = Arena(device, sum(Arena.room(b.nbytes, max(b.align, 256), b.guard) for b, _, _ in bufs.values()) + (1 << 16))
    handles = {}
    for name, (b, first, roles) in bufs.items():
        if arena is not None:
            h = arena.carve(name, b.nbytes, align=b.align, guard_after=b.guard,
                            role="zeroed" if "zeroed" in roles else ("scratch" if first == "zero_once" else first))
        else:
            h = _Plain(b, device)
        handles[name] = h
        if first in ("in", "inout"):
            assert b.data is not None, f"`{name}` is an input without data"
            h.put(b.data.to(device))
        elif first in ("zeroed", "zero_once"):
            h.set_bytes(0)
            if first == "zero_once" and scratch_fill is not None:      # only the block that stays zeroed carries anything
                h.u8()[b.stays_zero[0] + b.stays_zero[1]:] = scratch_fill
        elif first == "scratch" and scratch_fill is not None:
            h.set_bytes(scratch_fill)
        if b.zero_at is not None:
            h.u8()[b.zero_at[0]:b.zero_at[0] + b.zero_at[1]] = 0

    def addr(ref):
        return None if ref is None else handles[ref.buf.name].dptr + ref.offset

    lib = L.lib()
    for k, c in enumerate(calls):
        cargs, keep = marshal(c, addr)
        for h in handles.values():
            h.snapshot = None
        written = {r.buf.name for r in c.refs() if r.role != "in"}
        for r in c.refs():
            if r.role == "in" and r.buf.name not in written:
                handles[r.buf.name].freeze()
        rc = getattr(lib, c.entry)(*cargs, L.stream())
        torch.cuda.synchronize()
        where = f"call {k} ({c.entry})"
        assert rc == 0, f"{where} returned {rc}: {lib.plnerf_error_string(rc).decode()}"
        if arena is not None:
            problems = arena.problems()
            assert not problems, where + ":\n" + "\n".join(problems)
        for name, h in handles.items():
            b, _, roles = bufs[name]
            if arena is None:
                if h.snapshot is not None:
                    assert torch.equal(h.u8(), h.snapshot), f"{where}: input `{name}` modified"
                if "zeroed" in roles:
                    assert not bool(h.u8().any()), f"{where}: zeroed `{name}` left non-zero"
            if b.stays_zero is not None:
                assert _span_is_zero(h, b.stays_zero), f"{where}: `{name}` bytes {b.stays_zero} not left zeroed"
            if b.zero_at is not None:
                assert _span_is_zero(h, b.zero_at), f"{where}: `{name}` status word {b.zero_at} became non-zero"
    return {name: handles[name].u8().cpu() for name, (b, _, roles) in bufs.items() if roles & {"out", "inout"}}


def _first_diff(x, y, keep):
    bad = ((x != y) & keep).nonzero().reshape(-1)
    return None if bad.numel() == 0 else f"{int(bad.numel())} byte(s), first at offset {int(bad[0])}, last at {int(bad[-1])}"


def run_case(L, calls, device):
    """The three runs and the conditions on their results.  Returns the results of the first run."""
    bufs = case_buffers(calls)
    run_a = run_once(L, calls, 0x00, device)
    run_b = run_once(L, calls, 0xFF, device)
    plain = run_once(L, calls, None, device)
    for name, a in run_a.items():
        b = bufs[name][0]
        if b.opaque:
            continue
        size = DTYPES[b.dtype][1]
        words = a.numel() // 4
        loose = torch.zeros(words, dtype=torch.bool)      # words no condition is put on
        if b.pad is not None:
            loose |= b.pad.reshape(-1)
        keep_bytes = torch.ones(a.numel(), dtype=torch.bool)
        keep_bytes[:words * 4] = ~loose.repeat_interleave(4)
        for other, which in ((run_b[name], "scratch at 0x00 and at 0xFF"), (plain[name], "the arena and ordinary allocations")):
            if b.untouched is not None and which.startswith("the arena"):      # (untouched words of an ordinary allocation hold anything)
                keep = keep_bytes.clone()
                keep[:words * 4] &= ~b.untouched.reshape(-1).repeat_interleave(4)
            else:
                keep = keep_bytes
            diff = _first_diff(a, other, keep)
            assert diff is None, f"`{name}` differs between {which}: {diff}"
        for run in (a, run_b[name]):
            if size >= 4:
                stale = fill_words(run[:words * 4])
                if b.untouched is not None:
                    u = b.untouched.reshape(-1)
                    assert bool(stale[u].all()), f"`{name}`: {int((~stale[u]).sum())} word(s) outside the call's range were written"
                    stale = stale & ~u
                stale = stale & ~loose
                assert not bool(stale.any()), (f"`{name}`: {int(stale.sum())} word(s) of a documented output still hold the fill, "
                                               f"first at word {int(stale.nonzero()[0])}")
            if b.finite and b.dtype in ("f32", "f64"):
                values = run.view(DTYPES[b.dtype][0])
                ok = torch.isfinite(values)
                if b.dtype == "f32":
                    ok |= loose | (b.untouched.reshape(-1) if b.untouched is not None else False)
                assert bool(ok.all()), f"`{name}`: {int((~ok).sum())} non-finite result(s), first at element {int((~ok).nonzero()[0])}"
    return run_a


# ---- checks a CPU can make on a case (tests/test_containment_table.py) ---------------------------------------------------
def check_against_prototype(call, c_params, argtypes):
    """One Call against its header prototype (parameter C types, comments stripped) and its ctypes signature: the arity
    (without the stream), pointer or scalar per argument, and const pointers only ever read."""
    assert len(call.args) + 1 == len(c_params) == len(argtypes), (call.entry, len(call.args) + 1, len(c_params))
    for k, (a, c_type) in enumerate(zip(call.args, c_params)):
        pointer = c_type.replace("const", "").strip().endswith("*")
        where = (call.entry, k, c_type)
        if not pointer:
            assert isinstance(a, (int, float)) and not isinstance(a, bool), where
            if c_type.strip() in ("float", "double"):
                assert isinstance(a, (int, float)), where
            else:
                assert isinstance(a, int), where
            continue
        assert a is None or isinstance(a, (Ref, PtrTable, HostArray, Struct)), where
        if isinstance(a, Ref):
            const = c_type.strip().startswith("const")
            assert (a.role == "in") == const, (where, a.buf.name, a.role)
            element = c_type.replace("const", "").replace("*", "").strip()
            sizes = {"float": 4, "double": 8, "int": 4, "uint32_t": 4, "int64_t": 8, "uint8_t": 1, "uint16_t": 2}
            if element in sizes:
                assert DTYPES[a.buf.dtype][1] == sizes[element], (where, a.buf.name, a.buf.dtype)
                assert a.buf.align % sizes[element] == 0, (where, a.buf.name, a.buf.align)


# =======================================================================================================================
# The table.  One builder per family; a builder returns the list of Calls of ONE case.  Arguments stand in header order.
# =======================================================================================================================
MODE_CONSTANT, MODE_LINEAR = _lib.MODE["constant"], _lib.MODE["linear"]
# (header constants come from the binding, plnerf_amd._lib, which tests/test_abi_headers.py and the *_abi tests hold to
# the headers; sizes come from the size queries)
PRECISIONS = _lib.PRECISION
KERNEL_AUTO, KERNEL_RR, KERNEL_PP = (_lib.FWD_KERNELS[k] for k in ("auto", "rr", "pp"))
MAX_SAMPLES = _lib.DEPTH_STEP_MAX_SAMPLES      # PLNERF_MAX_SAMPLES
QUAD_GROUP = _lib.QUAD_RAYS_PER_GROUP
ZERO_TOL, EPSILON = 1e-4, 1e-3
SEED, STEP = 1234, 7


def _rays(tag, R):
    near = uniform(f"{tag}near", R, lo=2.0, hi=2.5)
    far = given(f"{tag}far", "f32", near.data + 4.0)
    rays_o = uniform(f"{tag}rays_o", R, 3, lo=-1.0, hi=1.0)
    d = torch.randn(R, 3, generator=_gen(f"{tag}rays_d"))
    d[:, 2] = -1.0 - d[:, 2].abs()      # (looking down -z, never a zero direction: plnerf_ndc_rays divides by d_z)
    return near, far, rays_o, given(f"{tag}rays_d", "f32", d)


def _raw(name, R, S):
    """The network's output [R,S,4], 16-byte aligned, with a density that stays positive under the noise: a ray without any
    density has acc_map = 0 and the reference's disparity 1 / max(1e-10, depth / acc) is then 0 / 0 -- NaN by its own
    formula, which would say nothing about the kernel under condition (f)."""
    raw = torch.randn(R, S, 4, generator=_gen(name))
    raw[..., 3] = raw[..., 3].abs() + 0.5
    return given(name, "f32", raw, align=16)


def draws_case(R, n):
    """plnerf_uniform, plnerf_normal: Philox yields four values per block, n = 1, 5, 10 end inside one."""
    return [Call("plnerf_uniform", SEED, 1, STEP, 3, R, n, OUT(out("uniform", "f32", R, n))),
            Call("plnerf_normal", SEED, 2, STEP, 3, R, n, OUT(out("normal", "f32", R, n)))]


def prologue_case(R, S, N):
    """plnerf_stratified_z, plnerf_ray_points, plnerf_coarse_samples (jitter given, and drawn in the kernel),
    plnerf_merge_sort: all take S >= 1."""
    near, far, rays_o, rays_d = _rays("", R)
    t_vals = given("t_vals", "f32", torch.linspace(0., 1., S))
    t_rand = uniform("t_rand", R, S)
    z = out("z_vals", "f32", R, S)
    z_new = uniform("z_new", R, N, lo=1.0, hi=7.5)      # (some outside [near, far]: the clamp)
    calls = [
        Call("plnerf_stratified_z", IN(near), IN(far), IN(t_vals), IN(t_rand), R, S, 0, OUT(z)),
        Call("plnerf_stratified_z", IN(near), IN(far), IN(t_vals), None, R, S, 1, OUT(out("z_lindisp", "f32", R, S))),
        Call("plnerf_ray_points", IN(rays_o), IN(rays_d), IN(z), R, S, OUT(out("pts", "f32", R, S, 3))),
        Call("plnerf_coarse_samples", IN(rays_o), IN(rays_d), IN(near), IN(far), IN(t_vals), IN(t_rand), SEED, STEP, 3, R, S, 0, 1,
             OUT(out("cs_z", "f32", R, S)), OUT(out("cs_pts", "f32", R, S, 3))),
        Call("plnerf_coarse_samples", IN(rays_o), IN(rays_d), IN(near), IN(far), IN(t_vals), None, SEED, STEP, 3, R, S, 1, 1,
             OUT(out("cs_z_drawn", "f32", R, S)), OUT(out("cs_pts_drawn", "f32", R, S, 3, align=16))),
        Call("plnerf_merge_sort", IN(z), IN(z_new), IN(near), IN(far), R, S, N, OUT(out("merged", "f32", R, S + N))),
    ]
    return calls


def linear_case(R, S, N, epilogues=True):
    """Piecewise-linear mode, S >= 2 (the quadrature and the epilogues refuse S < 2; the samplers alone run from S = 1 in
    pl_sampler_case): plnerf_quad_fwd / _bwd / _bwd_rays, plnerf_sample_pl / _bwd / _bwd_rays on the quadrature's own weights,
    plnerf_coarse_epilogue, plnerf_fine_epilogue -- each once with every optional pointer given and once
    with every optional pointer NULL.  The backwards read what the forwards of the same case wrote."""
    assert S >= 2
    near, far, rays_o, rays_d = _rays("", R)
    z = sorted_depths("z", near, far, R, S)
    raw = _raw("raw", R, S)
    noise = normal("noise", R, S, scale=0.1)
    u = uniform("u", R, N)
    u_row = given("u_row", "f32", torch.linspace(0., 1., N))
    q = (IN(raw), IN(z), IN(near), IN(far), IN(rays_d))
    flags = (R, S, MODE_LINEAR, 0, 1, 1)      # mode linear, colour midpoint, white background, farcolorfix
    weights, tau, T = out("weights", "f32", R, S + 1), out("tau", "f32", R, S + 2), out("T", "f32", R, S + 2)
    maps = lambda tag: [OUT(out(f"{tag}rgb", "f32", R, 3)), OUT(out(f"{tag}disp", "f32", R)), OUT(out(f"{tag}acc", "f32", R)),
                        OUT(out(f"{tag}depth", "f32", R))]
    samples, inds = out("samples", "f32", R, N), out("inds", "i64", R, N)
    g = {k: normal(f"g_{k}", *shape) for k, shape in (("rgb", (R, 3)), ("depth", (R,)), ("acc", (R,)), ("weights", (R, S + 1)),
                                                        ("samples", (R, N)))}
    g_tau, g_T = out("g_tau", "f32", R, S + 2), out("g_T", "f32", R, S + 2)
    groups = -(-R // QUAD_GROUP)
    pl = (IN(z), IN(tau), IN(T), IN(near), IN(far))
    calls = [
        Call("plnerf_quad_fwd", *q, IN(noise), *flags, *maps("q_"), OUT(weights), OUT(tau), OUT(T)),
        Call("plnerf_quad_fwd", *q, None, *flags, *maps("qn_"), None, None, None),
        Call("plnerf_sample_pl", IN(z), IN(weights), IN(tau), IN(T), IN(near), IN(far), IN(u), N, R, S, N, ZERO_TOL, EPSILON,
             OUT(samples), OUT(out("T_below", "f32", R, N)), OUT(out("tau_below", "f32", R, N)), OUT(out("bin_below", "f32", R, N)),
             OUT(inds)),
        Call("plnerf_sample_pl", IN(z), IN(weights), IN(tau), IN(T), IN(near), IN(far), IN(u_row), 0, R, S, N, ZERO_TOL, EPSILON,
             OUT(out("samples_row", "f32", R, N)), None, None, None, None),
        Call("plnerf_sample_pl_bwd", *pl, IN(u), N, IN(inds), IN(g["samples"]), R, S, N, ZERO_TOL, EPSILON, OUT(g_tau), OUT(g_T)),
        Call("plnerf_sample_pl_bwd_rays", *pl, IN(u), N, IN(inds), IN(g["samples"]), R, S, N, ZERO_TOL, EPSILON,
             OUT(out("gr_tau", "f32", R, S + 2)), OUT(out("gr_T", "f32", R, S + 2)), OUT(out("g_knots", "f32", R, S + 2))),
        Call("plnerf_quad_bwd", *q, IN(noise), *flags, IN(g["rgb"]), IN(g["depth"]), IN(g["acc"]), IN(g["weights"]), IN(g_tau), IN(g_T),
             OUT(out("g_raw", "f32", R, S, 4, align=16)), OUT(out("absmax", "u32", groups))),
        Call("plnerf_quad_bwd", *q, None, *flags, IN(g["rgb"]), None, None, None, None, None,
             OUT(out("g_raw_n", "f32", R, S, 4, align=16)), None),
        Call("plnerf_quad_bwd_rays", *q, IN(noise), *flags, IN(g["rgb"]), IN(g["depth"]), IN(g["acc"]), IN(g["weights"]), IN(g_tau),
             IN(g_T), OUT(out("gr_raw", "f32", R, S, 4, align=16)), OUT(out("g_z", "f32", R, S)), OUT(out("g_near", "f32", R)),
             OUT(out("g_far", "f32", R)), OUT(out("g_dnorm", "f32", R))),
    ]
    if epilogues:
        F = S + N
        rng = (SEED, STEP, 3, R, S, N, 0, 1, 1, ZERO_TOL, EPSILON)
        calls += [
            Call("plnerf_coarse_epilogue", *q[:4], IN(rays_o), IN(rays_d), IN(noise), IN(u), N, *rng, *maps("ce_"),
                 OUT(out("ce_weights", "f32", R, S + 1)), OUT(out("ce_tau", "f32", R, S + 2)), OUT(out("ce_T", "f32", R, S + 2)),
                 OUT(out("ce_z_fine", "f32", R, F)), OUT(out("ce_pts", "f32", R, F, 3)), OUT(out("ce_z_std", "f32", R))),
            Call("plnerf_coarse_epilogue", *q[:4], IN(rays_o), IN(rays_d), None, None, 0, *rng, *maps("cen_"), None, None, None,
                 OUT(out("cen_z_fine", "f32", R, F)), OUT(out("cen_pts", "f32", R, F, 3, align=16)), OUT(out("cen_z_std", "f32", R))),
            Call("plnerf_fine_epilogue", *q, IN(noise), IN(u_row), 0, *rng, *maps("fe_"), OUT(out("fe_weights", "f32", R, S + 1)),
                 OUT(out("fe_tau", "f32", R, S + 2)), OUT(out("fe_T", "f32", R, S + 2)), OUT(out("fe_samples", "f32", R, N)),
                 OUT(out("fe_inds", "i64", R, N)), OUT(out("fe_u", "f32", R, N)), OUT(out("fe_z_std", "f32", R))),
            Call("plnerf_fine_epilogue", *q, None, None, 0, *rng, *maps("fen_"), OUT(out("fen_weights", "f32", R, S + 1)),
                 OUT(out("fen_tau", "f32", R, S + 2)), OUT(out("fen_T", "f32", R, S + 2)), OUT(out("fen_samples", "f32", R, N)),
                 OUT(out("fen_inds", "i64", R, N)), None, OUT(out("fen_z_std", "f32", R))),
        ]
    return calls


def pl_sampler_case(R, S, N):
    """plnerf_sample_pl / _bwd / _bwd_rays from S = 1, the smallest knot row (two weights, three tau / T), which no
    quadrature can supply (it needs S >= 2): tau is a hand-made running sum of positive steps over the knots
    [near, z, far], T = exp(-tau), weights = T[k] - T[k + 1]."""
    near, far, _, _ = _rays("", R)
    z = sorted_depths("z", near, far, R, S)
    steps = torch.rand(R, S + 1, generator=_gen("tau_steps")) * 0.9 + 0.1
    tau_v = torch.cat([torch.zeros(R, 1), torch.cumsum(steps, dim=1)], dim=1)
    T_v = torch.exp(-tau_v)
    tau, T = given("tau", "f32", tau_v), given("T", "f32", T_v)
    weights = given("weights", "f32", T_v[:, :-1] - T_v[:, 1:])
    u, u_row = uniform("u", R, N), given("u_row", "f32", torch.linspace(0., 1., N))
    g_samples = normal("g_samples", R, N)
    inds = out("inds", "i64", R, N)
    pl = (IN(z), IN(tau), IN(T), IN(near), IN(far))
    return [
        Call("plnerf_sample_pl", IN(z), IN(weights), IN(tau), IN(T), IN(near), IN(far), IN(u), N, R, S, N, ZERO_TOL, EPSILON,
             OUT(out("samples", "f32", R, N)), OUT(out("T_below", "f32", R, N)), OUT(out("tau_below", "f32", R, N)),
             OUT(out("bin_below", "f32", R, N)), OUT(inds)),
        Call("plnerf_sample_pl", IN(z), IN(weights), IN(tau), IN(T), IN(near), IN(far), IN(u_row), 0, R, S, N, ZERO_TOL, EPSILON,
             OUT(out("samples_row", "f32", R, N)), None, None, None, None),
        Call("plnerf_sample_pl_bwd", *pl, IN(u), N, IN(inds), IN(g_samples), R, S, N, ZERO_TOL, EPSILON,
             OUT(out("g_tau", "f32", R, S + 2)), OUT(out("g_T", "f32", R, S + 2))),
        Call("plnerf_sample_pl_bwd_rays", *pl, IN(u), N, IN(inds), IN(g_samples), R, S, N, ZERO_TOL, EPSILON,
             OUT(out("gr_tau", "f32", R, S + 2)), OUT(out("gr_T", "f32", R, S + 2)), OUT(out("g_knots", "f32", R, S + 2))),
    ]


def constant_case(R, S, N, epilogues=True):
    """Piecewise-constant mode: the quadrature (from S = 2, the smallest it accepts) with plnerf_sample_const / _bwd on
    B = S bins (from B = 2, the smallest they accept), and -- from S = 3, the const stages need one interior weight --
    plnerf_coarse_epilogue_const, plnerf_fine_epilogue_const and its backward plnerf_fine_epilogue_const_bwd on what that
    forward wrote."""
    assert S >= 2
    near, far, rays_o, rays_d = _rays("", R)
    z = sorted_depths("z", near, far, R, S)
    raw = _raw("raw", R, S)
    noise = normal("noise", R, S, scale=0.1)
    u = uniform("u", R, N)
    u_row = given("u_row", "f32", torch.linspace(0., 1., N))
    q = (IN(raw), IN(z), IN(near), IN(far), IN(rays_d))
    flags = (R, S, MODE_CONSTANT, 0, 1, 0)
    maps = lambda tag: [OUT(out(f"{tag}rgb", "f32", R, 3)), OUT(out(f"{tag}disp", "f32", R)), OUT(out(f"{tag}acc", "f32", R)),
                        OUT(out(f"{tag}depth", "f32", R))]
    g = {k: normal(f"g_{k}", *shape) for k, shape in (("rgb", (R, 3)), ("depth", (R,)), ("acc", (R,)), ("weights", (R, S)),
                                                        ("samples", (R, N)))}
    groups = -(-R // QUAD_GROUP)
    B = S
    pdf_w = uniform("pdf_weights", R, B - 1, lo=0.0, hi=1.0)
    inds = out("sc_inds", "i64", R, N)
    calls = [
        Call("plnerf_quad_fwd", *q, IN(noise), *flags, *maps("q_"), OUT(out("weights", "f32", R, S)), None, None),
        Call("plnerf_quad_fwd", *q, None, *flags, *maps("qn_"), None, None, None),
        Call("plnerf_quad_bwd", *q, IN(noise), *flags, IN(g["rgb"]), IN(g["depth"]), IN(g["acc"]), IN(g["weights"]), None, None,
             OUT(out("g_raw", "f32", R, S, 4, align=16)), OUT(out("absmax", "u32", groups))),
        Call("plnerf_quad_bwd_rays", *q, None, *flags, IN(g["rgb"]), None, None, None, None, None,
             OUT(out("gr_raw", "f32", R, S, 4, align=16)), OUT(out("g_z", "f32", R, S)), OUT(out("g_near", "f32", R)),
             OUT(out("g_far", "f32", R)), OUT(out("g_dnorm", "f32", R))),
        Call("plnerf_sample_const", IN(z), IN(pdf_w), IN(u), N, R, B, N, OUT(out("sc_samples", "f32", R, N)), OUT(inds)),
        Call("plnerf_sample_const", IN(z), IN(pdf_w), IN(u_row), 0, R, B, N, OUT(out("sc_samples_row", "f32", R, N)), None),
        Call("plnerf_sample_const_bwd", IN(z), IN(pdf_w), IN(u), N, IN(inds), IN(g["samples"]), R, B, N,
             OUT(out("sc_g_weights", "f32", R, B - 1))),
    ]
    if epilogues and S >= 3:
        F = S + N
        rng = (SEED, STEP, 3, R, S, N, 1)
        fe_w, fe_bins = out("fe_weights", "f32", R, S), out("fe_bins", "f32", R, S - 1)
        fe_inds, fe_u = out("fe_inds", "i64", R, N), out("fe_u", "f32", R, N)
        calls += [
            Call("plnerf_coarse_epilogue_const", *q[:4], IN(rays_o), IN(rays_d), IN(noise), IN(u), N, *rng, *maps("ce_"),
                 OUT(out("ce_weights", "f32", R, S)), OUT(out("ce_z_fine", "f32", R, F)), OUT(out("ce_pts", "f32", R, F, 3)),
                 OUT(out("ce_z_std", "f32", R))),
            Call("plnerf_coarse_epilogue_const", *q[:4], IN(rays_o), IN(rays_d), None, None, 0, *rng, *maps("cen_"), None,
                 OUT(out("cen_z_fine", "f32", R, F)), OUT(out("cen_pts", "f32", R, F, 3, align=16)), OUT(out("cen_z_std", "f32", R))),
            Call("plnerf_fine_epilogue_const", *q, IN(noise), None, 0, *rng, *maps("fe_"), OUT(fe_w), OUT(fe_bins),
                 OUT(out("fe_samples", "f32", R, N)), OUT(fe_inds), OUT(fe_u), OUT(out("fe_z_std", "f32", R))),
            Call("plnerf_fine_epilogue_const", *q, None, IN(u_row), 0, *rng, *maps("fen_"), OUT(out("fen_weights", "f32", R, S)), None,
                 OUT(out("fen_samples", "f32", R, N)), OUT(out("fen_inds", "i64", R, N)), None, OUT(out("fen_z_std", "f32", R))),
            Call("plnerf_fine_epilogue_const_bwd", *q, IN(noise), IN(fe_w), IN(fe_bins), IN(fe_u), N, IN(fe_inds), R, S, N, 1,
                 IN(g["rgb"]), IN(g["depth"]), IN(g["acc"]), IN(g["weights"]), IN(g["samples"]),
                 OUT(out("feb_g_raw", "f32", R, S, 4, align=16)), OUT(out("feb_absmax", "u32", groups))),
            Call("plnerf_fine_epilogue_const_bwd", *q, None, None, None, None, 0, None, R, S, N, 1, IN(g["rgb"]), None, None, None, None,
                 OUT(out("febn_g_raw", "f32", R, S, 4, align=16)), None),
        ]
    return calls


def ray_selection_case(R):
    """plnerf_select_rays, plnerf_view_rays, plnerf_ndc_rays, plnerf_select_bank_rays, plnerf_select_depth_rays on 9 x 11
    views (99 pixels >= 67 rays), each with its nullable outputs given and NULL."""
    H, W, V, n_hyp = 9, 11, 2, 3
    K = (12.5, 11.5, 5.5, 4.5)
    c2w = [0.8, -0.6, 0.0, 0.5, 0.6, 0.8, 0.0, -0.25, 0.0, 0.0, 1.0, 4.0]
    image = uniform("image", H, W, 3)
    near, far, rays_o, rays_d = _rays("in_", R)
    images3 = uniform("bank_images", 3, H, W, 3)
    poses3 = given("bank_c2w", "f32", torch.tensor(c2w).repeat(3, 1) + 0.01 * torch.arange(3.)[:, None])
    views = given("bank_views", "i32", torch.tensor([2, 0]))
    rays = lambda t: [OUT(out(f"{t}rays_o", "f32", R, 3)), OUT(out(f"{t}rays_d", "f32", R, 3))]
    nf = lambda t: [OUT(out(f"{t}near", "f32", R)), OUT(out(f"{t}far", "f32", R))]
    d_images, d_hyp = uniform("d_images", V, H, W, 3), uniform("d_hyp", V, n_hyp, H, W, lo=2.0, hi=6.0)
    d_valid = given("d_valid", "u8", (torch.rand(V, H, W, generator=_gen("d_valid")) > 0.3))
    d_poses4 = given("d_poses4", "f32", torch.cat([torch.tensor(c2w).view(3, 4), torch.tensor([[0., 0., 0., 1.]])]).repeat(V, 1, 1))
    d_poses3 = given("d_poses3", "f32", torch.tensor(c2w).view(3, 4).repeat(V, 1, 1))
    d_K = given("d_intrinsics", "f32", torch.tensor(K).repeat(V, 1))
    d_scale, d_shift = uniform("d_scale", V, lo=0.9, hi=1.1), uniform("d_shift", V, lo=-0.1, hi=0.1)
    return [
        Call("plnerf_select_rays", H, W, *K, HostArray(ctypes.c_float, c2w), IN(image), 1, 2, 8, 9, SEED, STEP, 3, R, 2.0, 6.0,
             *rays("sr_"), OUT(out("sr_viewdirs", "f32", R, 3)), *nf("sr_"), OUT(out("sr_target", "f32", R, 3)),
             OUT(out("sr_pixels", "i32", R, 2))),
        Call("plnerf_select_rays", H, W, *K, HostArray(ctypes.c_float, c2w), None, 0, 0, H, W, SEED, STEP, 0, R, 2.0, 6.0,
             *rays("srn_"), None, *nf("srn_"), None, None),
        Call("plnerf_view_rays", H, W, *K, HostArray(ctypes.c_float, c2w), 99 - R, R, 2.0, 6.0, *rays("vr_"),
             OUT(out("vr_viewdirs", "f32", R, 3)), *nf("vr_")),
        Call("plnerf_view_rays", H, W, *K, HostArray(ctypes.c_float, c2w), 0, R, 2.0, 6.0, *rays("vrn_"), None, *nf("vrn_")),
        Call("plnerf_ndc_rays", H, W, 12.5, 1.0, IN(rays_o), IN(rays_d), R, OUT(out("ndc_o", "f32", R, 3)), OUT(out("ndc_d", "f32", R, 3))),
        Call("plnerf_select_bank_rays", 2, IN(views), H, W, *K, IN(poses3), IN(images3), SEED, 1, 2 * H * W - R, R, 2.0, 6.0,
             *rays("br_"), OUT(out("br_viewdirs", "f32", R, 3)), *nf("br_"), OUT(out("br_target", "f32", R, 3)),
             OUT(out("br_index", "i32", R))),
        Call("plnerf_select_bank_rays", 2, IN(views), H, W, *K, IN(poses3), None, SEED, 0, 0, R, 2.0, 6.0, *rays("brn_"), None,
             *nf("brn_"), None, None),
        Call("plnerf_select_depth_rays", V, 1, H, W, n_hyp, IN(d_images), IN(d_hyp), IN(d_valid), IN(d_poses4), 4, IN(d_K), IN(d_scale),
             IN(d_shift), 2.0, 6.0, SEED, STEP, H * W - R, R, *rays("dr_"), OUT(out("dr_viewdirs", "f32", R, 3)), *nf("dr_"),
             OUT(out("dr_target", "f32", R, 3)), OUT(out("dr_target_h", "f32", n_hyp, R)), OUT(out("dr_mask", "f32", R)),
             OUT(out("dr_hyp_raw", "f32", n_hyp, R)), OUT(out("dr_pixels", "i32", R, 2))),
        Call("plnerf_select_depth_rays", V, 0, H, W, n_hyp, IN(d_images), IN(d_hyp), None, IN(d_poses3), 3, IN(d_K), None, None,
             2.0, 6.0, SEED, STEP, 0, R, *rays("drn_"), None, *nf("drn_"), OUT(out("drn_target", "f32", R, 3)),
             OUT(out("drn_target_h", "f32", n_hyp, R)), OUT(out("drn_mask", "f32", R)), None, None),
    ]


def embed_case(n_rays, spr):
    """plnerf_embed_rows: the NVS encoding (10 | 4 bands -> 63 | 27), the depth script's (9 | 0 -> 57 | 3, scale pi, a
    bounding box), one with a camera code behind it, and the position block alone."""
    n = n_rays * spr
    pts, dirs = uniform("pts", n, 3, lo=-1.5, hi=1.5), normal("viewdirs", n_rays, 3)
    cam = normal("cam", 4)
    return [
        Call("plnerf_embed_rows", IN(pts), IN(dirs), None, n, spr, 10, 4, 0, 1.0, None, 1.0, OUT(out("emb_nvs", "f32", n, 90))),
        Call("plnerf_embed_rows", IN(pts), IN(dirs), None, n, spr, 9, 0, 0, math.pi, HostArray(ctypes.c_float, [0.1, -0.2, 0.3]), 0.5,
             OUT(out("emb_depth", "f32", n, 60))),
        Call("plnerf_embed_rows", IN(pts), IN(dirs), IN(cam), n, spr, 9, 0, 4, math.pi, None, 1.0, OUT(out("emb_cam", "f32", n, 64))),
        Call("plnerf_embed_rows", IN(pts), None, None, n, spr, 10, 0, 0, 1.0, None, 1.0, OUT(out("emb_xyz", "f32", n, 63))),
    ]


def losses_case(R, P, joint):
    """plnerf_image_loss (two images; then the fine image alone with an earlier coarse term), plnerf_depth_loss,
    plnerf_depth_joint_sums, plnerf_depth_scale_shift_grad: R rays, P points, three hypotheses, in a view of four.  The
    loss workspaces are `zeroed`: zero before the call and zero again after it."""
    n_hyp, V = 3, 4
    rgb, rgb0, target = uniform("rgb", R, 3), uniform("rgb0", R, 3), uniform("target", R, 3)
    pred = uniform("pred_hyp", R, P, lo=2.0, hi=6.0)
    target_h = uniform("target_h", n_hyp, R, P, lo=2.0, hi=6.0)
    target_h1 = uniform("target_h1", n_hyp, R, 1, lo=2.0, hi=6.0)
    hyp_raw = uniform("hyp_raw", n_hyp, R, P, lo=2.0, hi=6.0)
    mask = given("mask", "f32", (torch.rand(R, generator=_gen("mask")) > 0.25).float())
    il_ws = out("image_loss_ws", "u8", _lib.IMAGE_LOSS_WORKSPACE_BYTES, align=8)
    dl_ws = out("depth_loss_ws", "u8", _lib.DEPTH_LOSS_WORKSPACE_BYTES, align=8)
    coarse = out("coarse_loss4", "f32", 4)
    choice = given("joint_choice", "i32", torch.arange(P) % n_hyp)
    calls = [
        Call("plnerf_image_loss", IN(rgb), IN(rgb0), IN(target), R, OUT(out("loss4", "f32", 4)), OUT(out("il_g_rgb", "f32", R, 3)),
             OUT(out("il_g_rgb0", "f32", R, 3)), None, ZEROED(il_ws)),
        Call("plnerf_image_loss", IN(rgb0), None, IN(target), R, OUT(coarse), OUT(out("ilc_g_rgb", "f32", R, 3)), None, None,
             ZEROED(il_ws)),
        Call("plnerf_image_loss", IN(rgb), None, IN(target), R, OUT(out("loss4_late", "f32", 4)), OUT(out("ill_g_rgb", "f32", R, 3)), None,
             IN(coarse), ZEROED(il_ws)),
        Call("plnerf_depth_loss", IN(rgb), IN(rgb0), IN(target), IN(pred), IN(target_h), IN(mask), R, P, n_hyp, P, joint, None, 0.007,
             0.05, OUT(out("loss5", "f32", 5)), OUT(out("dl_g_rgb", "f32", R, 3)), OUT(out("dl_g_rgb0", "f32", R, 3)),
             OUT(out("dl_g_hyp", "f32", R, P)), ZEROED(dl_ws)),
        Call("plnerf_depth_loss", IN(rgb), None, IN(target), IN(pred), IN(target_h1), None, R, P, n_hyp, 1, joint,
             IN(choice) if joint else None, 0.007, 0.05, OUT(out("loss5_n", "f32", 5)), OUT(out("dln_g_rgb", "f32", R, 3)), None,
             OUT(out("dln_g_hyp", "f32", R, P)), ZEROED(dl_ws)),
        Call("plnerf_depth_loss", IN(rgb), None, IN(target), None, None, None, R, P, n_hyp, P, 0, None, 0.007, 0.05,
             OUT(out("loss5_warm", "f32", 5)), OUT(out("dlw_g_rgb", "f32", R, 3)), None, None, ZEROED(dl_ws)),
        Call("plnerf_depth_joint_sums", IN(pred), IN(target_h), IN(mask), R, P, n_hyp, P, 0.05, OUT(out("joint_sums", "f64", n_hyp, P))),
        Call("plnerf_depth_joint_sums", IN(pred), IN(target_h1), None, R, P, n_hyp, 1, 0.05, OUT(out("joint_sums1", "f64", n_hyp, P))),
        Call("plnerf_depth_scale_shift_grad", IN(pred), IN(target_h), IN(hyp_raw), IN(mask), R, P, n_hyp, P, joint,
             IN(choice) if joint else None, 0.007, 0.05, V, 2, OUT(out("g_scale", "f32", V)), OUT(out("g_shift", "f32", V)),
             SCRATCH(out("ss_ws", "u8", _lib.DEPTH_SS_WORKSPACE_BYTES, align=8))),
        Call("plnerf_depth_scale_shift_grad", IN(pred), IN(target_h), IN(hyp_raw), None, R, P, n_hyp, P, joint, None, 0.007, 0.05, V, 0,
             OUT(out("g_scale_n", "f32", V)), OUT(out("g_shift_n", "f32", V)), SCRATCH(out("ss_ws_n", "u8", _lib.DEPTH_SS_WORKSPACE_BYTES, align=8))),
    ]
    return calls


def gemm_case(M, N, K, k_splits):
    """plnerf_gemm_f32 into a C of row stride ldc = N + 5 -- the five columns behind every row stay untouched -- with bias and
    ReLU, and the transposed-A / gate / ones-column form of the weight gradient (A read as [K, M] through swapped strides),
    partials of exactly k_splits * M * N floats."""
    ldc = N + 5
    a, b, bias = normal("a", M, K), normal("b", K, N), normal("bias", N)
    at, gate = normal("a_t", K, M), normal("gate", K, M)
    behind = torch.zeros(M, ldc, dtype=torch.bool)
    behind[:, N:] = True
    partials = lambda name: SCRATCH(out(name, "f32", k_splits, M, N)) if k_splits > 1 else None
    return [
        Call("plnerf_gemm_f32", IN(a), K, 1, IN(b), N, 1, IN(bias), None, M, N, K, 1, 0, 0,
             OUT(out("c", "f32", M, ldc, untouched=behind)), ldc, k_splits, partials("partials")),
        Call("plnerf_gemm_f32", IN(at), 1, M, IN(b), N, 1, None, IN(gate), M, N, K, 0, 0, 1,
             OUT(out("c_wgrad", "f32", M, ldc, untouched=behind)), ldc, k_splits, partials("partials_wgrad")),
    ]


def adam_case(n, guarded):
    """plnerf_adam_step on exactly n floats per buffer, without and with the guard words (both zero: the step happens and
    the withheld counter stays what it was), and plnerf_depth_ss_adam on n views."""
    p = lambda t: [INOUT(normal(f"{t}param", n)), IN(normal(f"{t}grad", n, scale=0.1)), INOUT(normal(f"{t}m", n, scale=0.01)),
                   INOUT(uniform(f"{t}v", n, lo=0.0, hi=1e-3))]
    word = lambda name, v: given(name, "u32", torch.tensor([v]))
    guards = [IN(word("skip1", 0)), IN(word("skip2", 0)), INOUT(word("withheld", 5))] if guarded else [None, None, None]
    return [
        Call("plnerf_adam_step", *p(""), n, 5e-4, 0.9, 0.999, 1e-8, 3, 0.5, 0.1, *guards),
        Call("plnerf_depth_ss_adam", INOUT(uniform("scale", n, lo=0.9, hi=1.1)), INOUT(uniform("shift", n, lo=-0.1, hi=0.1)),
             IN(normal("ss_grad", 2, n, scale=0.1)), INOUT(normal("ss_m", 2, n, scale=0.01)), INOUT(uniform("ss_v", 2, n, lo=0.0, hi=1e-3)),
             n, 1e-3, 0.9, 0.999, 1e-8, 2, 1.0),
    ]


def eval_case(n, H, W):
    """plnerf_eval_metrics with a workspace of exactly PLNERF_EVAL_WORKSPACE_BYTES(n, H, W), with and without pred0 and the
    depth triple (without pred0 the header defines column PLNERF_EVAL_SSE_RGB0 as NaN)."""
    ws_bytes = _lib.eval_workspace_bytes(n, H, W)
    pred, target, pred0 = uniform("pred", n, H, W, 3, lo=-0.1, hi=1.1), uniform("target", n, H, W, 3), uniform("pred0", n, H, W, 3)
    depth, tdepth = uniform("depth", n, H, W, lo=2.0, hi=6.0), uniform("target_depth", n, H, W, lo=2.0, hi=6.0)
    valid = given("valid", "u8", torch.rand(n, H, W, generator=_gen("valid")) > 0.3)
    return [
        Call("plnerf_eval_metrics", n, H, W, IN(pred), IN(target), IN(pred0), IN(depth), IN(tdepth), IN(valid),
             SCRATCH(out("eval_ws", "u8", ws_bytes, align=8)), OUT(out("rows", "f64", n, _lib.EVAL_ROW))),
        Call("plnerf_eval_metrics", n, H, W, IN(pred), IN(target), None, None, None, None,
             SCRATCH(out("eval_ws_n", "u8", ws_bytes, align=8)), OUT(out("rows_n", "f64", n, _lib.EVAL_ROW, finite=False))),
    ]


def sample_error_case(L, R, N):
    """plnerf_sample_error with a workspace of exactly plnerf_sample_error_workspace_bytes(R): written, then accumulated
    into; with and without `valid`."""
    ws_bytes = int(L.lib().plnerf_sample_error_workspace_bytes(R))
    pred, depth = uniform("pred_hyp", R, N, lo=2.0, hi=6.0), uniform("depth", R, lo=2.0, hi=6.0)
    valid = given("valid", "u8", torch.rand(R, generator=_gen("valid")) > 0.3 if R > 1 else torch.ones(1, dtype=torch.bool))
    ws, row = out("se_ws", "u8", ws_bytes, align=8), out("se_row", "f64", 2)
    return [
        Call("plnerf_sample_error", R, N, IN(pred), IN(depth), IN(valid), 0, SCRATCH(ws), OUT(row)),
        Call("plnerf_sample_error", R, N, IN(pred), IN(depth), None, 1, SCRATCH(ws), INOUT(row)),
    ]


# ---- the MLP family ------------------------------------------------------------------------------------------------------
def param_shapes(input_ch, input_ch_views):
    """The 24 parameter tensors in state_dict order (plnerf_hip.h)."""
    shapes = []
    for layer in range(8):
        fan_in = input_ch if layer == 0 else (256 + input_ch if layer == 5 else 256)
        shapes += [(256, fan_in), (256,)]
    return shapes + [(128, 256 + input_ch_views), (128,), (256, 256), (256,), (1, 256), (1,), (3, 128), (3,)]


def network(tag, input_ch, input_ch_views):
    """One network's parameters as ONE flat buffer in state_dict order (optim.FlatAdam's layout: rgb_linear.weight then
    starts 4 bytes off a 16-byte boundary, feature_linear on one), torch-like initial values; returns (flat Buf, byte
    offsets, element counts)."""
    shapes = param_shapes(input_ch, input_ch_views)
    g = _gen(f"{tag}params")
    parts = []
    for shape in shapes:
        fan_in = shape[1] if len(shape) == 2 else 256
        parts.append(((torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan_in)).reshape(-1))
    parts[21] = torch.ones(1)      # alpha_linear.bias: a density that is positive somewhere along every ray (see _raw)
    counts = [p.numel() for p in parts]
    offsets = [4 * sum(counts[:k]) for k in range(24)]
    assert (input_ch, input_ch_views) != (63, 27) or sum(counts) == 595844      # PLNERF_N_PARAMS
    return given(f"{tag}param_flat", "f32", torch.cat(parts), align=16), offsets, counts


def _tile_guards(L, precision):
    """The bytes one full workgroup tile of the widest writer covers, from the layout constants through the size queries:
    256 rows of saved state (the forward's largest tile) and 192 rows of the backward's workspace (the dgrad tile)."""
    lib = L.lib()
    saved = int(lib.plnerf_mlp_saved_bytes(256, precision)) - int(lib.plnerf_mlp_saved_bytes(0, precision))
    bwd = int(lib.plnerf_mlp_bwd_workspace_bytes(192, precision)) - int(lib.plnerf_mlp_bwd_workspace_bytes(0, precision))
    return saved, bwd


def _packed(L, tag, precision):
    lib = L.lib()
    nbytes, status = int(lib.plnerf_mlp_packed_bytes(precision)), int(lib.plnerf_mlp_status_offset(precision))
    # the weight sections, every word of them written by plnerf_mlp_pack_weights, then the 16-byte status block: the word
    # the caller zeroes and three words nothing touches
    assert nbytes == status + 16
    behind = torch.zeros(nbytes // 4, dtype=torch.bool)
    behind[status // 4 + 1:] = True
    return out(f"{tag}packed", "u32", nbytes // 4, align=256, untouched=behind, zero_at=(status, 4))


RELU_MASK_BYTES = 272      # SV_MASK_BYTES of mlp_layout.h (no query or header exposes it; tests/test_host_cpu.py::test_buffer_size_queries
                           # holds the size queries to the same number)


def _saved(L, name, n_rows, precision, guard):
    """The saved state: in the exact-fp32 mode exactly n_rows rows; in the 16-bit modes rows padded to 256 ("written, never
    read") in a layout private to the library: opaque."""
    nbytes = int(L.lib().plnerf_mlp_saved_bytes(n_rows, precision))
    if precision == PRECISIONS["fp32"]:
        assert nbytes == n_rows * int(L.lib().plnerf_mlp_saved_bytes(1, precision))      # exactly n_rows rows
        # [planes: 2528 floats per row, every one written][272 bytes per row: the section of the 16-bit kernels' ReLU bit
        # masks, which the size query counts in every mode and the fp32 kernels neither write nor read (plnerf_hip.h)]
        words = nbytes // 4
        unused = torch.zeros(words, dtype=torch.bool)
        unused[words - n_rows * (RELU_MASK_BYTES // 4):] = True
        return out(name, "u32", words, align=256, guard=guard, pad=unused)
    return out(name, "u8", nbytes, align=256, guard=guard, opaque=True)


def _grads(tag, counts):
    """24 gradient tensors carved at their exact sizes, each at the 4-byte alignment the header allows."""
    return [out(f"{tag}grad{k:02d}", "f32", n) for k, n in enumerate(counts)]


def mlp_case(L, precision, fwd_kernel, route, n_rows, density_beta, absmax):
    """plnerf_mlp_pack_weights -> plnerf_mlp_fwd (inference, saved NULL) -> plnerf_mlp_fwd (training, saved of exactly
    plnerf_mlp_saved_bytes) -> plnerf_mlp_bwd (workspace of exactly plnerf_mlp_bwd_workspace_bytes, 24 gradients at their
    exact sizes) -> plnerf_mlp_input_grad on that workspace.  route: "pts" (63 | 27, encoding in the kernel), "emb" (63 | 27,
    caller-embedded) or "emb57" (57 | 3, caller-embedded).  absmax: hand the backward max |g_raw| as three candidates
    (16-bit modes without a density activation), else NULL."""
    lib = L.lib()
    P = PRECISIONS[precision]
    ich, vch = (57, 3) if route == "emb57" else (63, 27)
    embedded = route != "pts"
    spr = 4
    n_rays = -(-n_rows // spr)
    flat, offs, counts = network("", ich, vch)
    params = PtrTable([IN(flat, o) for o in offs])
    packed = _packed(L, "", P)
    saved_guard, bwd_guard = _tile_guards(L, P)
    saved = _saved(L, "saved", n_rows, P, saved_guard)
    ws = out("bwd_ws", "u8", int(lib.plnerf_mlp_bwd_workspace_bytes(n_rows, P)), align=256, guard=bwd_guard, opaque=True)
    layout = int(lib.plnerf_mlp_saved_layout(P, int(embedded), fwd_kernel))
    assert layout >= 0
    if embedded:
        x = (None, None, IN(normal("embedded", n_rows, ich + vch, scale=0.5)))
    else:
        x = (IN(uniform("pts", n_rows, 3, lo=-1.5, hi=1.5)), IN(normal("viewdirs", n_rays, 3)), None)
    raw_out = out("raw_out", "f32", n_rows, 4, align=16)
    g_raw = normal("g_raw", n_rows, 4, scale=0.01, align=16)
    use_absmax = absmax and P != 0 and density_beta == 0
    if use_absmax:      # three candidates whose maximum is the fp32 bit pattern of max |g_raw| (plnerf_quad_bwd's absmax_out)
        top = g_raw.data.abs().max()
        cand = given("g_absmax", "u32", torch.stack([top * 0.5, top, top * 0.25]).view(torch.int32))
    grads = _grads("", counts)
    return [
        Call("plnerf_mlp_pack_weights", params, P, ich, vch, OUT(packed)),
        Call("plnerf_mlp_fwd", IN(packed), P, *x, ich, vch, n_rows, spr, 1.0, density_beta, OUT(out("raw_infer", "f32", n_rows, 4, align=16)),
             None, fwd_kernel),
        Call("plnerf_mlp_fwd", IN(packed), P, *x, ich, vch, n_rows, spr, 1.0, density_beta, OUT(raw_out), OUT(saved), fwd_kernel),
        Call("plnerf_mlp_bwd", IN(packed), P, IN(g_raw), IN(cand) if use_absmax else None, 3 if use_absmax else 0, ich, vch, n_rows,
             IN(saved), layout, IN(raw_out) if density_beta > 0 else None, density_beta, SCRATCH(ws),
             PtrTable([OUT(b) for b in grads]), OUT(out("status_out", "f32", 1)) if absmax else None),
        Call("plnerf_mlp_input_grad", params, P, ich, vch, n_rows, IN(ws), OUT(out("g_embedded", "f32", n_rows, ich + vch, guard=256 * (ich + vch) * 4))),      # (guard: a 256-row tile of its writer)
    ]


def mlp_multi_case(L, precision, rows):
    """plnerf_mlp_bwd_multi: two jobs of unequal rows on one network, each with its own exact-size saved state, workspace
    and 24 gradient tensors; max |g_raw| handed over for the second job only, status_out for the first only."""
    lib = L.lib()
    P = PRECISIONS[precision]
    flat, offs, counts = network("", 63, 27)
    params = PtrTable([IN(flat, o) for o in offs])
    packed = _packed(L, "", P)
    saved_guard, bwd_guard = _tile_guards(L, P)
    layout = int(lib.plnerf_mlp_saved_layout(P, 0, KERNEL_AUTO))
    calls = [Call("plnerf_mlp_pack_weights", params, P, 63, 27, OUT(packed))]
    jobs = []
    for j, n in enumerate(rows):
        saved = _saved(L, f"saved{j}", n, P, saved_guard)
        ws = out(f"bwd_ws{j}", "u8", int(lib.plnerf_mlp_bwd_workspace_bytes(n, P)), align=256, guard=bwd_guard, opaque=True)
        g_raw = normal(f"g_raw{j}", n, 4, scale=0.01, align=16)
        calls.append(Call("plnerf_mlp_fwd", IN(packed), P, IN(uniform(f"pts{j}", n, 3, lo=-1.5, hi=1.5)),
                          IN(normal(f"viewdirs{j}", -(-n // 4), 3)), None, 63, 27, n, 4, 1.0, 0.0, OUT(out(f"raw_out{j}", "f32", n, 4, align=16)),
                          OUT(saved), KERNEL_AUTO))
        top = g_raw.data.abs().max()
        jobs.append((saved, ws, g_raw, given(f"g_absmax{j}", "u32", torch.stack([top, top * 0.5]).view(torch.int32)),
                     _grads(f"j{j}_", counts)))
    hand_over = P != 0
    calls.append(Call(
        "plnerf_mlp_bwd_multi", 2, PtrTable([IN(packed), IN(packed)]), P, PtrTable([IN(j[2]) for j in jobs]),
        PtrTable([None, IN(jobs[1][3])]) if hand_over else None, HostArray(ctypes.c_int, [0, 2]) if hand_over else None, 63, 27,
        HostArray(ctypes.c_int, rows), PtrTable([IN(j[0]) for j in jobs]), HostArray(ctypes.c_int, [layout, layout]), None, 0.0,
        PtrTable([SCRATCH(j[1]) for j in jobs]), PtrTable([OUT(b) for j in jobs for b in j[4]]),
        PtrTable([OUT(out("status_out0", "f32", 1)), None])))
    return calls


# ---- the one-call entries ------------------------------------------------------------------------------------------------
ONE_CALL_RAYS, ONE_CALL_SAMPLES, ONE_CALL_IMPORTANCE = 67, 16, 16      # the issue's aim; every size query accepts it
ONE_CALL_H, ONE_CALL_W = 9, 11
ONE_CALL_C2W = [0.8, -0.6, 0.0, 0.5, 0.6, 0.8, 0.0, -0.25, 0.0, 0.0, 1.0, 4.0]


def _step_config(L, mode, precision, max_rays=ONE_CALL_RAYS, perturb=1, noise=1.0):
    cfg = L.StepConfig()
    cfg.max_rays, cfg.n_samples, cfg.n_importance = max_rays, ONE_CALL_SAMPLES, ONE_CALL_IMPORTANCE
    cfg.mode, cfg.color_mode, cfg.lindisp, cfg.perturb, cfg.white_bkgd, cfg.farcolorfix = mode, 0, 0, perturb, 1, 0
    cfg.raw_noise_std, cfg.zero_tol, cfg.epsilon, cfg.ndc, cfg.ndc_focal = noise, ZERO_TOL, EPSILON, 0, 12.5
    cfg.H, cfg.W, cfg.fx, cfg.fy, cfg.cx, cfg.cy = ONE_CALL_H, ONE_CALL_W, 12.5, 11.5, 5.5, 4.5
    cfg.near, cfg.far, cfg.precision, cfg.fwd_kernel, cfg.input_ch, cfg.input_ch_views = 2.0, 6.0, PRECISIONS[precision], 0, 63, 27
    cfg.ray_source, cfg.n_views, cfg.beta1, cfg.beta2, cfg.adam_eps, cfg.seed, cfg.bank_seed = 0, 0, 0.9, 0.999, 1e-8, SEED, 0
    return cfg


class _Net:
    """One network of a one-call step: parameters, gradient block (n + 4 floats: [n] the range status, the other three
    documented as unused), Adam moments and packed buffer, all carved at their exact sizes."""

    def __init__(self, L, tag, precision, train=True):
        self.flat, self.offs, counts = network(tag, 63, 27)
        self.n = sum(counts)
        self.packed = _packed(L, tag, PRECISIONS[precision])
        if train:
            tail = torch.zeros(self.n + 4, dtype=torch.bool)
            tail[self.n + 1:] = True
            self.grad = out(f"{tag}grad_flat", "f32", self.n + 4, align=16, pad=tail)
            self.m = given(f"{tag}exp_avg", "f32", torch.zeros(self.n), align=16)
            self.v = given(f"{tag}exp_avg_sq", "f32", torch.zeros(self.n), align=16)

    def train_refs(self):
        return [INOUT(self.flat), OUT(self.grad), INOUT(self.m), INOUT(self.v), OUT(self.packed)]

    def fill_step_net(self, net, addr):
        base = addr(INOUT(self.flat))
        for k, o in enumerate(self.offs):
            net.params[k] = base + o
        net.param_flat, net.grad_flat, net.exp_avg, net.exp_avg_sq = base, addr(OUT(self.grad)), addr(INOUT(self.m)), addr(INOUT(self.v))
        net.n_params, net.packed = self.n, addr(OUT(self.packed))

    def view_refs(self):
        return [IN(self.flat), OUT(self.packed)]

    def fill_view_net(self, net, addr):
        base = addr(IN(self.flat))
        for k, o in enumerate(self.offs):
            net.params[k] = base + o
        net.packed = addr(OUT(self.packed))


def train_step_case(L, mode, precision="f16x3"):
    """plnerf_train_step (mode linear) / plnerf_train_step_const (constant): two steps of 67 then 41 rays, 16 + 16 samples,
    density noise and jitter on, on a workspace of EXACTLY the size query's bytes at 256-byte alignment, zeroed once; the
    loss kernel's partials (its first PLNERF_IMAGE_LOSS_WORKSPACE_BYTES) must be zero again after every step."""
    entry = "plnerf_train_step" if mode == MODE_LINEAR else "plnerf_train_step_const"
    cfg = _step_config(L, mode, precision)
    nbytes = int(getattr(L.lib(), entry + "_workspace_bytes")(ctypes.byref(cfg)))
    assert nbytes > 0, "the size query refuses 67 rays of 16 + 16 samples"
    saved_guard, bwd_guard = _tile_guards(L, cfg.precision)
    ws = out("workspace", "u8", nbytes, align=256, guard=max(saved_guard, bwd_guard), opaque=True, stays_zero=(0, _lib.IMAGE_LOSS_WORKSPACE_BYTES))
    coarse, fine = _Net(L, "c_", precision), _Net(L, "f_", precision)
    t_vals = given("t_vals", "f32", torch.linspace(0., 1., ONE_CALL_SAMPLES))
    u_vals = given("u_vals", "f32", torch.linspace(0., 1., ONE_CALL_IMPORTANCE))
    image = uniform("image", ONE_CALL_H, ONE_CALL_W, 3)
    calls = []
    for step, rays in ((0, ONE_CALL_RAYS), (1, 41)):
        loss4 = out(f"loss4_step{step}", "f32", 4)

        def build_io(addr, loss4=loss4):
            io = L.StepIo()
            coarse.fill_step_net(io.coarse, addr)
            fine.fill_step_net(io.fine, addr)
            io.t_vals, io.u_vals, io.loss4 = addr(IN(t_vals)), addr(IN(u_vals)), addr(OUT(loss4))
            return io

        def build_args(addr, step=step, rays=rays):
            a = L.StepArgs()
            a.rays, a.step, a.ray_id0 = rays, step, 5 * step
            a.c2w[:] = ONE_CALL_C2W
            a.image = addr(IN(image))
            a.crop_r0, a.crop_c0, a.crop_rows, a.crop_cols = 0, 0, ONE_CALL_H, ONE_CALL_W
            a.lr_fine, a.lr_coarse, a.adam_step_fine, a.adam_step_coarse, a.loss_scale = 5e-4, 5e-4, step + 1, step + 1, 1.0
            return a

        calls.append(Call(entry, Struct([], lambda addr: cfg), Struct(coarse.train_refs() + fine.train_refs() +
                                                                       [IN(t_vals), IN(u_vals), OUT(loss4)], build_io),
                          Struct([IN(image)], build_args), ZERO_ONCE(ws), nbytes))
    return calls


DEPTH_VIEWS, DEPTH_HYP = 2, 3


def depth_step_config(L, precision):
    V, H, W, n_hyp = DEPTH_VIEWS, ONE_CALL_H, ONE_CALL_W, DEPTH_HYP
    cfg = L.DepthStepConfig()
    cfg.max_rays, cfg.n_samples, cfg.n_importance = ONE_CALL_RAYS, ONE_CALL_SAMPLES, ONE_CALL_IMPORTANCE
    cfg.color_mode, cfg.lindisp, cfg.perturb, cfg.white_bkgd, cfg.raw_noise_std = 0, 0, 1, 0, 1.0
    cfg.zero_tol, cfg.epsilon, cfg.n_views, cfg.H, cfg.W, cfg.n_hyp, cfg.pose_rows = ZERO_TOL, EPSILON, V, H, W, n_hyp, 3
    cfg.near, cfg.far, cfg.precision, cfg.fwd_kernel, cfg.input_ch, cfg.input_ch_views = 2.0, 6.0, PRECISIONS[precision], 0, 63, 27
    cfg.input_scale, cfg.density_beta, cfg.is_joint = 1.0, 10.0, 0
    cfg.space_carving_weight, cfg.space_carving_threshold, cfg.clip_value = 0.007, 0.0, 0.1
    cfg.beta1, cfg.beta2, cfg.adam_eps, cfg.ss_beta1, cfg.ss_beta2, cfg.ss_adam_eps, cfg.seed = 0.9, 0.999, 1e-8, 0.9, 0.999, 1e-8, SEED
    return cfg


def depth_step_case(L, constant, precision="f16x3"):
    """plnerf_depth_train_step / plnerf_depth_train_step_const: two steps of 67 then 41 rays of view 1 of two 9 x 11 views
    with three hypotheses, 16 + 16 samples, the in-kernel encoding (63 | 27) with the softplus density (beta 10), space
    carving on; the second step also steps the depth scales and shifts.  Workspace as train_step_case (PLNERF_DEPTH_LOSS_WORKSPACE_BYTES first)."""
    entry = "plnerf_depth_train_step_const" if constant else "plnerf_depth_train_step"
    V, H, W, n_hyp = DEPTH_VIEWS, ONE_CALL_H, ONE_CALL_W, DEPTH_HYP
    cfg = depth_step_config(L, precision)
    nbytes = int(getattr(L.lib(), entry + "_workspace_bytes")(ctypes.byref(cfg)))
    assert nbytes > 0, "the size query refuses 67 rays of 16 + 16 samples"
    saved_guard, bwd_guard = _tile_guards(L, cfg.precision)
    ws = out("workspace", "u8", nbytes, align=256, guard=max(saved_guard, bwd_guard), opaque=True, stays_zero=(0, _lib.DEPTH_LOSS_WORKSPACE_BYTES))
    coarse, fine = _Net(L, "c_", precision), _Net(L, "f_", precision)
    t_vals = given("t_vals", "f32", torch.linspace(0., 1., ONE_CALL_SAMPLES))
    u_vals = given("u_vals", "f32", torch.linspace(0., 1., ONE_CALL_IMPORTANCE))
    images, hyp = uniform("images", V, H, W, 3), uniform("hyp", V, n_hyp, H, W, lo=2.0, hi=6.0)
    valid = given("valid", "u8", torch.rand(V, H, W, generator=_gen("valid")) > 0.3)
    poses = given("poses", "f32", torch.tensor(ONE_CALL_C2W).view(3, 4).repeat(V, 1, 1))
    intrinsics = given("intrinsics", "f32", torch.tensor([12.5, 11.5, 5.5, 4.5]).repeat(V, 1))
    scale, shift = uniform("scale", V, lo=0.9, hi=1.1), uniform("shift", V, lo=-0.1, hi=0.1)
    ss_grad = out("ss_grad", "f32", 2, V)
    ss_m, ss_v = given("ss_exp_avg", "f32", torch.zeros(2, V)), given("ss_exp_avg_sq", "f32", torch.zeros(2, V))
    ins = [IN(t_vals), IN(u_vals), IN(images), IN(hyp), IN(valid), IN(poses), IN(intrinsics)]
    calls = []
    for step, rays in ((0, ONE_CALL_RAYS), (1, 41)):
        loss5 = out(f"loss5_step{step}", "f32", 5)
        # (a step without ss_step reads scale and shift and leaves the three optimizer arrays alone)
        ss = [INOUT(scale), INOUT(shift), OUT(ss_grad), INOUT(ss_m), INOUT(ss_v)] if step else [IN(scale), IN(shift)]

        def build_io(addr, loss5=loss5, step=step):
            io = L.DepthStepIo()
            coarse.fill_step_net(io.coarse, addr)
            fine.fill_step_net(io.fine, addr)
            (io.t_vals, io.u_vals, io.images, io.hyp, io.valid, io.poses, io.intrinsics) = [addr(r) for r in ins]
            io.scale, io.shift = addr(IN(scale)), addr(IN(shift))
            if step:
                io.ss_grad, io.ss_exp_avg, io.ss_exp_avg_sq = addr(OUT(ss_grad)), addr(INOUT(ss_m)), addr(INOUT(ss_v))
            io.loss5 = addr(OUT(loss5))
            return io

        def build_args(addr, step=step, rays=rays):
            a = L.DepthStepArgs()
            a.view, a.rays, a.step, a.ray_id0, a.lr, a.adam_step = 1, rays, step, 5 * step, 5e-4, step + 1
            a.carve, a.ss_step, a.ss_lr, a.ss_adam_step = 1, step, 1e-3, 1
            return a

        calls.append(Call(entry, Struct([], lambda addr: cfg),
                          Struct(coarse.train_refs() + fine.train_refs() + ins + ss + [OUT(loss5)], build_io),
                          Struct([], build_args), ZERO_ONCE(ws), nbytes))
    return calls


def render_view_case(L, mode, precision="f16x3"):
    """plnerf_render_view on a 9 x 11 view in blocks of 32 pixels (99 = 3 * 32 + 3): the whole frame with every plane and
    both exports, then pixels [5, 45) with every nullable plane left out -- the frame's other pixels stay untouched.  The
    workspace is exactly the size query's bytes, and need not be zeroed: scratch."""
    cfg = _step_config(L, mode, precision, max_rays=32, perturb=0, noise=0.0)
    nbytes = int(L.lib().plnerf_render_view_workspace_bytes(ctypes.byref(cfg)))
    assert nbytes > 0
    ws = out("workspace", "u8", nbytes, align=256, opaque=True)
    coarse, fine = _Net(L, "c_", precision, train=False), _Net(L, "f_", precision, train=False)
    t_vals = given("t_vals", "f32", torch.linspace(0., 1., ONE_CALL_SAMPLES))
    u_vals = given("u_vals", "f32", torch.linspace(0., 1., ONE_CALL_IMPORTANCE))
    n = ONE_CALL_H * ONE_CALL_W
    planes = {name: out(f"plane_{name}", "f32", *((n, 3) if name in ("rgb", "rgb0") else (n,))) for name in L.VIEW_PLANES}
    rgb8, depth16 = out("rgb8", "u8", n, 3), out("depth16", "u16", n)
    outside = torch.ones(n, 3, dtype=torch.bool)
    outside[5:45] = False
    part = out("part_rgb", "f32", n, 3, untouched=outside)
    nets = coarse.view_refs() + fine.view_refs() + [IN(t_vals), IN(u_vals)]

    def build_io(addr, full):
        io = L.ViewIo()
        coarse.fill_view_net(io.coarse, addr)
        fine.fill_view_net(io.fine, addr)
        io.t_vals, io.u_vals = addr(IN(t_vals)), addr(IN(u_vals))
        if full:
            for name in L.VIEW_PLANES:
                setattr(io, name, addr(OUT(planes[name])))
            io.rgb8, io.depth16 = addr(OUT(rgb8)), addr(OUT(depth16))
        else:
            io.rgb = addr(OUT(part))
        return io

    def build_args(addr, full):
        a = L.ViewArgs()
        a.c2w[:] = ONE_CALL_C2W
        a.step, a.pix0, a.n_pix, a.pack_weights, a.depth16_scale = 3, 0 if full else 5, n if full else 40, 1, 1.0 / 6.0
        return a

    return [
        Call("plnerf_render_view", Struct([], lambda addr: cfg),
             Struct(nets + [OUT(p) for p in planes.values()] + [OUT(rgb8), OUT(depth16)], lambda addr: build_io(addr, True)),
             Struct([], lambda addr: build_args(addr, True)), SCRATCH(ws), nbytes),
        Call("plnerf_render_view", Struct([], lambda addr: cfg), Struct(nets + [OUT(part)], lambda addr: build_io(addr, False)),
             Struct([], lambda addr: build_args(addr, False)), SCRATCH(ws), nbytes),
    ]


# ---- refusals: a float4 array that is not 16-byte aligned ---------------------------------------------------------------
EINVAL = -1


def misaligned_cases(L, shift=4):
    """Every entry that takes raw, g_raw or raw_out [n,4], or feature_linear's weight / bias, handed that pointer 4 bytes
    off a 16-byte boundary: (id, [Call]) -- each call must return PLNERF_EINVAL and write nothing.  shift = 0 gives the same
    calls with that pointer aligned: the control that shows nothing else about them is refused."""
    R, S, N = 5, 8, 4
    near, far, rays_o, rays_d = _rays("", R)
    z = sorted_depths("z", near, far, R, S)
    raw_ok = normal("raw", R, S, 4, align=16)
    raw_off = normal("raw_off", R * S * 4 + 4, align=16)
    g_rgb = normal("g_rgb", R, 3)
    maps = lambda t: [OUT(out(f"{t}rgb", "f32", R, 3)), OUT(out(f"{t}disp", "f32", R)), OUT(out(f"{t}acc", "f32", R)),
                      OUT(out(f"{t}depth", "f32", R))]
    graw_off = lambda t: OUT(out(f"{t}g_raw_off", "f32", R * S * 4 + 4, align=16), shift)
    rest = (IN(z), IN(near), IN(far))
    lin, con = (R, S, MODE_LINEAR, 0, 1, 0), (R, S, MODE_CONSTANT, 0, 1, 0)
    none5 = (None,) * 5
    rng = (SEED, STEP, 0, R, S, N)
    F = S + N
    wtt = lambda t: [OUT(out(f"{t}w", "f32", R, S + 1)), OUT(out(f"{t}tau", "f32", R, S + 2)), OUT(out(f"{t}T", "f32", R, S + 2))]
    fine_tail = lambda t: [OUT(out(f"{t}samples", "f32", R, N)), OUT(out(f"{t}inds", "i64", R, N)), None, OUT(out(f"{t}z_std", "f32", R))]
    coarse_tail = lambda t: [OUT(out(f"{t}z_fine", "f32", R, F)), OUT(out(f"{t}pts", "f32", R, F, 3)), OUT(out(f"{t}z_std", "f32", R))]
    cases = [
        ("quad_fwd-raw", [Call("plnerf_quad_fwd", IN(raw_off, shift), *rest, IN(rays_d), None, *lin, *maps("a_"), None, None, None)]),
        ("quad_bwd-raw", [Call("plnerf_quad_bwd", IN(raw_off, shift), *rest, IN(rays_d), None, *con, IN(g_rgb), *none5,
                               OUT(out("b_g_raw", "f32", R, S, 4, align=16)), None)]),
        ("quad_bwd-g_raw", [Call("plnerf_quad_bwd", IN(raw_ok), *rest, IN(rays_d), None, *lin, IN(g_rgb), *none5, graw_off("c_"), None)]),
        ("quad_bwd_rays-g_raw", [Call("plnerf_quad_bwd_rays", IN(raw_ok), *rest, IN(rays_d), None, *lin, IN(g_rgb), *none5, graw_off("d_"),
                                      OUT(out("d_g_z", "f32", R, S)), OUT(out("d_g_near", "f32", R)), OUT(out("d_g_far", "f32", R)),
                                      OUT(out("d_g_dnorm", "f32", R)))]),
        ("coarse_epilogue-raw", [Call("plnerf_coarse_epilogue", IN(raw_off, shift), *rest, IN(rays_o), IN(rays_d), None, None, 0, *rng, 0, 1, 0,
                                      ZERO_TOL, EPSILON, *maps("e_"), None, None, None, *coarse_tail("e_"))]),
        ("fine_epilogue-raw", [Call("plnerf_fine_epilogue", IN(raw_off, shift), *rest, IN(rays_d), None, None, 0, *rng, 0, 1, 0, ZERO_TOL,
                                    EPSILON, *maps("f_"), *wtt("f_"), *fine_tail("f_"))]),
        ("coarse_epilogue_const-raw", [Call("plnerf_coarse_epilogue_const", IN(raw_off, shift), *rest, IN(rays_o), IN(rays_d), None, None, 0,
                                            *rng, 1, *maps("g_"), None, *coarse_tail("g_"))]),
        ("fine_epilogue_const-raw", [Call("plnerf_fine_epilogue_const", IN(raw_off, shift), *rest, IN(rays_d), None, None, 0, *rng, 1,
                                          *maps("h_"), OUT(out("h_w", "f32", R, S)), None, *fine_tail("h_"))]),
        ("fine_epilogue_const_bwd-raw", [Call("plnerf_fine_epilogue_const_bwd", IN(raw_off, shift), *rest, IN(rays_d), None, None, None, None, 0,
                                              None, R, S, N, 1, IN(g_rgb), None, None, None, None,
                                              OUT(out("i_g_raw", "f32", R, S, 4, align=16)), None)]),
        ("fine_epilogue_const_bwd-g_raw", [Call("plnerf_fine_epilogue_const_bwd", IN(raw_ok), *rest, IN(rays_d), None, None, None, None, 0,
                                                None, R, S, N, 1, IN(g_rgb), None, None, None, None, graw_off("j_"), None)]),
    ]
    # the MLP entries, f16x3 and fp32: raw_out of the forward; g_raw and raw_out of the backward; feature_linear of the pack
    lib = L.lib()
    n = 33
    for precision in ("f16x3", "fp32"):
        P = PRECISIONS[precision]
        t = precision + "_"
        flat, offs, counts = network(t, 63, 27)
        # the same network with feature_linear.weight (18) / .bias (19) moved 4 bytes: one spare float ahead of each
        shifted = given(f"{t}shifted_flat", "f32", torch.cat([flat.data, torch.zeros(8)]), align=16)
        params = lambda move: PtrTable([IN(shifted, o + (shift if k == move else 0)) for k, o in enumerate(offs)])
        packed = _packed(L, t, P)
        saved = _saved(L, f"{t}saved", n, P, 0)
        ws = out(f"{t}bwd_ws", "u8", int(lib.plnerf_mlp_bwd_workspace_bytes(n, P)), align=256, opaque=True)
        layout = int(lib.plnerf_mlp_saved_layout(P, 0, KERNEL_AUTO))
        pts, dirs = uniform(f"{t}pts", n, 3), normal(f"{t}viewdirs", n, 3)
        g_ok, g_off = normal(f"{t}g_raw", n, 4, align=16), normal(f"{t}g_raw_off", n * 4 + 4, align=16)
        ro_ok, ro_off = normal(f"{t}raw_out", n, 4, align=16), normal(f"{t}raw_out_off", n * 4 + 4, align=16)
        grads = lambda tag: PtrTable([OUT(b) for b in _grads(f"{t}{tag}", counts)])
        bwd = lambda g, ro, beta, tag: Call("plnerf_mlp_bwd", IN(packed), P, g, None, 0, 63, 27, n, IN(saved), layout, ro, beta,
                                            SCRATCH(ws), grads(tag), None)
        cases += [
            (f"pack-{precision}-feature_weight", [Call("plnerf_mlp_pack_weights", params(18), P, 63, 27, OUT(packed))]),
            (f"pack-{precision}-feature_bias", [Call("plnerf_mlp_pack_weights", params(19), P, 63, 27, OUT(packed))]),
            (f"fwd-{precision}-raw_out", [Call("plnerf_mlp_fwd", IN(packed), P, IN(pts), IN(dirs), None, 63, 27, n, 1, 1.0, 0.0,
                                               OUT(out(f"{t}fwd_raw_out_off", "f32", n * 4 + 4, align=16), shift), None, KERNEL_AUTO)]),
            (f"bwd-{precision}-g_raw", [bwd(IN(g_off, shift), None, 0.0, "a")]),
            (f"bwd-{precision}-raw_out", [bwd(IN(g_ok), IN(ro_off, shift), 10.0, "b")]),
            (f"bwd_multi-{precision}-second_g_raw", [Call(
                "plnerf_mlp_bwd_multi", 2, PtrTable([IN(packed), IN(packed)]), P, PtrTable([IN(g_ok), IN(g_off, shift)]), None, None, 63, 27,
                HostArray(ctypes.c_int, [n, n]), PtrTable([IN(saved), IN(saved)]), HostArray(ctypes.c_int, [layout, layout]), None, 0.0,
                PtrTable([SCRATCH(ws), SCRATCH(out(f"{t}bwd_ws2", "u8", ws.nbytes, align=256, opaque=True))]),
                PtrTable([OUT(b) for tag in ("c", "d") for b in _grads(f"{t}{tag}", counts)]), None)]),
        ]
    return cases


def _fake_addresses(calls):
    bufs = case_buffers(calls)
    fake = {name: (1 << 20) * (k + 1) for k, name in enumerate(bufs)}
    return lambda ref: None if ref is None else fake[ref.buf.name] + ref.offset


def refused_on_fake_pointers(L, calls):
    """The same calls without a device: every buffer gets a made-up address of its alignment (no refused call reads it), so
    the refusal is seen to come before anything touches a device -- a launch on a machine without one is PLNERF_ELAUNCH."""
    addr = _fake_addresses(calls)
    for c in calls:
        cargs, keep = marshal(c, addr)
        rc = getattr(L.lib(), c.entry)(*cargs, None)
        assert rc == EINVAL, (c.entry, rc)


def accepted_on_fake_pointers(L, calls):
    """The control of refused_on_fake_pointers: the aligned calls pass every argument check (on a machine without a device
    the launch then fails: PLNERF_ELAUNCH, anything but PLNERF_EINVAL).  ONLY without a device -- with one, a call that
    passes its checks would launch on made-up addresses; there the aligned control is every case of the table, on real memory."""
    assert not torch.cuda.is_available()
    addr = _fake_addresses(calls)
    for c in calls:
        cargs, keep = marshal(c, addr)
        rc = getattr(L.lib(), c.entry)(*cargs, None)
        assert rc != EINVAL and rc < 0, (c.entry, rc)


def run_refused(L, calls, device):
    """Carry out calls that must all be refused: PLNERF_EINVAL, every guard intact, every input unchanged, and every output
    still holding the fill -- a refused call has enqueued nothing."""
    bufs = case_buffers(calls)
    arena = Arena(device, sum(Arena.room(b.nbytes, max(b.align, 256), b.guard) for b, _, _ in bufs.values()) + (1 << 16))
    handles = {}
    for name, (b, first, roles) in bufs.items():
        handles[name] = arena.carve(name, b.nbytes, align=b.align, guard_after=b.guard, role="out" if first == "scratch" else first)
        if first == "in":
            if b.data is not None:      # (an opaque input of a call that is never made stays at the fill)
                handles[name].put(b.data.to(device))
            handles[name].freeze()
    lib = L.lib()
    addr = lambda ref: None if ref is None else handles[ref.buf.name].dptr + ref.offset
    for c in calls:
        cargs, keep = marshal(c, addr)
        rc = getattr(lib, c.entry)(*cargs, L.stream())
        torch.cuda.synchronize()
        assert rc == EINVAL, (c.entry, rc)
    arena.check()
    for name, (b, first, roles) in bufs.items():
        if first != "in":
            assert bool((handles[name].u8() == FILL).all()), f"`{name}` was written by a refused call"


# ---- every case, by family: (id, builder(L)) ---------------------------------------------------------------------------
RAYS = (1, 5, 67)
SAMPLES = (1, 37, 64)          # S; EACH entry runs at the smallest of these its own host check accepts, else at the nearest
                               # size it does: the quadrature (both modes), the linear epilogues and plnerf_sample_const
                               # (B) at 2, the constant-mode stages at 3
NEW_SAMPLES = (1, 5, 64)       # N
MLP_ROWS = (1, 33, 191, 193, 257, 577)      # 32-row MFMA tiles, the 192-row dgrad tile, the 256-row forward tile, and 577
MLP_ROUTES = ("pts", "emb", "emb57")
MLP_KERNELS = {"fp32": (KERNEL_AUTO,), "bf16x3": (KERNEL_RR, KERNEL_PP), "bf16": (KERNEL_RR, KERNEL_PP),
               "f16x3": (KERNEL_RR, KERNEL_PP), "f16": (KERNEL_RR, KERNEL_PP)}


def ray_cases():
    cases = []
    for R in RAYS:
        for n in (1, 5, 10):
            cases.append((f"draws-R{R}-n{n}", lambda L, R=R, n=n: draws_case(R, n)))
        for S in SAMPLES:
            for N in NEW_SAMPLES:
                cases.append((f"prologue-R{R}-S{S}-N{N}", lambda L, R=R, S=S, N=N: prologue_case(R, S, N)))
                cases.append((f"pl_sampler-R{R}-S{S}-N{N}", lambda L, R=R, S=S, N=N: pl_sampler_case(R, S, N)))
                cases.append((f"linear-R{R}-S{max(S, 2)}-N{N}", lambda L, R=R, S=S, N=N: linear_case(R, max(S, 2), N)))
                # (constant mode at S = 2: the quadrature and the sampler alone; from S = 3 with the one-launch stages)
                for Sc in ((2, 3) if S < 3 else (S,)):
                    cases.append((f"constant-R{R}-S{Sc}-N{N}", lambda L, R=R, S=Sc, N=N: constant_case(R, S, N)))
        cases.append((f"selection-R{R}", lambda L, R=R: ray_selection_case(R)))
        cases.append((f"embed-R{R}", lambda L, R=R: embed_case(R, 5)))
        for P in NEW_SAMPLES:
            for joint in (0, 1):
                cases.append((f"losses-R{R}-P{P}-joint{joint}", lambda L, R=R, P=P, joint=joint: losses_case(R, P, joint)))
    # S = PLNERF_MAX_SAMPLES: the quadrature and the samplers (the one-launch stages' LDS rows end below it)
    cases.append((f"linear-R3-S{MAX_SAMPLES}-N5", lambda L: linear_case(3, MAX_SAMPLES, 5, epilogues=False)))
    cases.append((f"constant-R3-S{MAX_SAMPLES}-N5", lambda L: constant_case(3, MAX_SAMPLES, 5, epilogues=False)))
    return cases


def other_cases():
    cases = []
    for shape in ((65, 63, 17), (3, 700, 90)):
        for k_splits in (1, 7):
            cases.append((f"gemm-{shape[0]}x{shape[1]}x{shape[2]}-k{k_splits}", lambda L, s=shape, k=k_splits: gemm_case(*s, k)))
    for n in (1, 255, 257):
        for guarded in (0, 1):
            cases.append((f"adam-n{n}-guard{guarded}", lambda L, n=n, g=guarded: adam_case(n, g)))
    for shape in ((2, 7, 7), (1, 37, 70)):
        cases.append((f"eval-{shape[0]}x{shape[1]}x{shape[2]}", lambda L, s=shape: eval_case(*s)))
    for R in (1, 67):
        cases.append((f"sample_error-R{R}", lambda L, R=R: sample_error_case(L, R, 5)))
    return cases


def mlp_cases(precision, fwd_kernel):
    """Every route and row count of one (precision, forward kernel); the density activation and the handed-over maximum
    alternate so that each row count and each route meets both."""
    cases = []
    for r, route in enumerate(MLP_ROUTES):
        for k, n_rows in enumerate(MLP_ROWS):
            beta = 10.0 if (r + k) % 2 else 0.0
            absmax = (r + k // 2) % 2 == 0
            cases.append((f"mlp-{precision}-k{fwd_kernel}-{route}-n{n_rows}-beta{int(beta)}-absmax{int(absmax)}",
                          lambda L, route=route, n=n_rows, beta=beta, absmax=absmax:
                          mlp_case(L, precision, fwd_kernel, route, n, beta, absmax)))
    return cases


def mlp_multi_cases(precision):
    return [(f"mlp_multi-{precision}-{a}+{b}", lambda L, rows=(a, b): mlp_multi_case(L, precision, rows))
            for a, b in ((193, 257), (1, 577))]


def one_call_cases():
    return [("train_step", lambda L: train_step_case(L, MODE_LINEAR)),
            ("train_step_const", lambda L: train_step_case(L, MODE_CONSTANT)),
            ("depth_train_step", lambda L: depth_step_case(L, False)),
            ("depth_train_step_const", lambda L: depth_step_case(L, True)),
            ("render_view-linear", lambda L: render_view_case(L, MODE_LINEAR)),
            ("render_view-constant", lambda L: render_view_case(L, MODE_CONSTANT))]


def all_cases():
    cases = ray_cases() + other_cases() + one_call_cases()
    for precision, kernels in MLP_KERNELS.items():
        for k in kernels:
            cases += mlp_cases(precision, k)
        cases += mlp_multi_cases(precision)
    return cases
