"""plnerf_amd.onecall's config fillers and the plan keys built from the same tuples, without a GPU and without the library:
a field that several of the one-call config structs carry is written alike into all of them, a filler writes nothing but
its own fields, the defaults are the documented ones, and a key tells two configurations apart."""
import ctypes

import pytest
import torch

SAMPLING = ("n_samples", "n_importance", "color_mode", "lindisp", "perturb", "white_bkgd", "raw_noise_std", "zero_tol", "epsilon")
NETWORK = ("max_rays", "precision", "fwd_kernel", "input_ch", "input_ch_views", "seed")
PINHOLE = ("ndc", "ndc_focal", "H", "W", "fx", "fy", "cx", "cy", "near", "far")
K = [[11.5, 0, 4.25], [0, 9.75, 6.5], [0, 0, 1]]
FULL = dict(N_samples=6, N_importance=5, color_mode="left", lindisp=True, perturb=1.0, white_bkgd=True, raw_noise_std=0.5,
            zero_tol=0.25, epsilon=0.125, farcolorfix=True)


@pytest.fixture(scope="module")
def nets():
    import plnerf_amd as P
    torch.manual_seed(0)
    return [P.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True, precision="f16x3")
            for _ in range(2)]


def _fields(struct):
    return [name for name, _ in struct._fields_]


def _values(cfg, names):
    return {name: getattr(cfg, name) for name in names}


def _filled(kw, coarse):
    """A StepConfig, a DepthStepConfig and a DepthViewConfig through the shared sampling filler alone."""
    from plnerf_amd import _lib as L, onecall
    cfgs = (L.StepConfig(), L.DepthStepConfig(), L.DepthViewConfig())
    for cfg in cfgs:
        onecall.fill_sampling(cfg, kw, 96, coarse, 2 ** 40 + 7)
    return cfgs


def test_shared_fields_are_filled_alike_and_from_kw(nets):
    from plnerf_amd import _lib as L
    cfgs = _filled(FULL, nets[0])
    common = set(_fields(cfgs[0])) & set(_fields(cfgs[1])) & set(_fields(cfgs[2]))
    assert common >= set(SAMPLING + NETWORK)
    written = set(SAMPLING + NETWORK)
    first = _values(cfgs[0], common)
    for cfg in cfgs[1:]:
        assert _values(cfg, common) == first
    f32 = lambda x: ctypes.c_float(x).value
    assert _values(cfgs[0], SAMPLING + NETWORK) == dict(
        n_samples=6, n_importance=5, color_mode=L.COLOR["left"], lindisp=1, perturb=1, white_bkgd=1, raw_noise_std=f32(0.5),
        zero_tol=f32(0.25), epsilon=f32(0.125), max_rays=96, precision=L.PRECISION["f16x3"], fwd_kernel=L.FWD_KERNEL, input_ch=63,
        input_ch_views=27, seed=2 ** 40 + 7)
    assert cfgs[0].farcolorfix == 1                                   # (written where the struct has it)
    for cfg in cfgs:                                                  # nothing else was touched, `mode` included: none was given
        others = [name for name in _fields(cfg) if name not in written and name != "farcolorfix"]
        assert others and all(getattr(cfg, name) == 0 for name in others), type(cfg).__name__


def test_each_filler_writes_its_own_fields_only(nets):
    from plnerf_amd import _lib as L, onecall
    f32 = lambda x: ctypes.c_float(x).value
    cfg = L.StepConfig()
    onecall.fill_pinhole(cfg, True, K, 13, 9, 2.0, 6.0)
    assert _values(cfg, PINHOLE) == dict(ndc=1, ndc_focal=11.5, H=13, W=9, fx=11.5, fy=9.75, cx=4.25, cy=6.5, near=2.0, far=6.0)
    assert all(getattr(cfg, name) == 0 for name in _fields(cfg) if name not in PINHOLE)
    group = {"betas": (0.8, 0.95), "eps": 1e-7}
    for cfg in (L.StepConfig(), L.DepthStepConfig()):
        onecall.fill_adam(cfg, group)
        assert (cfg.beta1, cfg.beta2, cfg.adam_eps) == (f32(0.8), f32(0.95), f32(1e-7))
        assert all(getattr(cfg, name) == 0 for name in _fields(cfg) if name not in ("beta1", "beta2", "adam_eps"))
    import plnerf_amd as P
    softplus = P.NeRF(input_ch=57, input_ch_views=3, use_viewdirs=True, density_activation="softplus")
    assert softplus.density_beta == 10.0 and nets[0].density_beta == 0.0
    for cfg in (L.DepthStepConfig(), L.DepthViewConfig()):
        onecall.fill_depth(cfg, 0.5, softplus)
        assert (cfg.input_scale, cfg.density_beta) == (0.5, 10.0)
        assert all(getattr(cfg, name) == 0 for name in _fields(cfg) if name not in ("input_scale", "density_beta"))
    cfg = L.DepthViewConfig()
    onecall.fill_sampling(cfg, FULL, 96, nets[0], 1, mode="linear")
    assert cfg.mode == L.MODE["linear"] != 0


def test_defaults_are_the_documented_ones(nets):
    from plnerf_amd import _lib as L
    f32 = lambda x: ctypes.c_float(x).value
    for cfg in _filled(dict(N_samples=6, N_importance=5), nets[0]):
        assert _values(cfg, SAMPLING[2:]) == dict(color_mode=L.COLOR["midpoint"], lindisp=0, perturb=0, white_bkgd=0,
                                                  raw_noise_std=0.0, zero_tol=f32(1e-4), epsilon=f32(1e-3))
        assert getattr(cfg, "farcolorfix", 0) == 0


def test_plan_keys_tell_sampling_fields_apart():
    from argparse import Namespace
    from plnerf_amd import stepplan
    args, views = Namespace(), object()
    keys = lambda kw: (stepplan.plan_key(kw, "view", 96, 13, 9, K, 2.0, 6.0, None, 3),
                       stepplan.depth_plan_key(args, kw, 96, views, 3))
    base = keys(FULL)
    assert keys(dict(FULL)) == base and hash(base[0]) == hash(keys(dict(FULL))[0])
    other = dict(N_samples=7, N_importance=4, color_mode="midpoint", lindisp=False, perturb=0.0, white_bkgd=False,
                 raw_noise_std=0.25, zero_tol=0.5, epsilon=0.25)
    assert set(other) == set(FULL) - {"farcolorfix"}
    for name, value in other.items():
        got = keys(dict(FULL, **{name: value}))
        assert got[0] != base[0] and got[1] != base[1], name
    assert keys(dict(FULL, farcolorfix=False))[0] != base[0]          # (a field of plnerf_step_config alone)
    assert stepplan.plan_key(FULL, "view", 96, 13, 9, K, 2.0, 6.5, None, 3) != base[0]
