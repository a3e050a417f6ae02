"""tests/exact_grid_cases.py without a GPU: the builder at every row count and seed tests/test_gpu_exact_grid.py uses, so the
conditions its bitwise comparisons rest on (the module's docstring, a-d; build() asserts them) are checked wherever the suite
runs."""
import numpy as np
import pytest

import exact_grid_cases as C
from oracle import plnerf_oracle as orc


def test_the_cases_cover_the_tile_edges():
    assert C.ROWS == (1, 33, 64, 65, 193, 257, 1000)
    assert set(C.TWO_JOBS) <= set(C.CASES) and {n for n, seed in C.CASES if seed == C.SEED} == set(C.ROWS)
    assert C.TWO_JOBS[0][1] != C.TWO_JOBS[1][1]


@pytest.mark.parametrize("seed", sorted({seed for _, seed in C.CASES}))
def test_the_network_is_sparse_and_signed(seed):
    sd = C.network(seed)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == orc.param_shapes()
    for name, w in sd.items():
        w = w.numpy()
        assert set(np.unique(w)) <= {-1.0, 0.0, 1.0}, name
        if w.ndim == 2:
            nnz = C.HEAD_NNZ if name.startswith(("alpha_linear", "rgb_linear")) else C.HIDDEN_NNZ
            assert ((w != 0).sum(1) == nnz).all() and (w == 1).any() and (w == -1).any(), name
        else:
            assert w.size < 128 or {-1.0, 0.0, 1.0} == set(np.unique(w)), name


@pytest.mark.parametrize("n,seed", C.CASES)
def test_the_arithmetic_is_exact_on_this_case(n, seed):
    """build() asserts a-d; here what it returns, and the rows' own pattern."""
    c = C.build(n, seed)
    assert c.embedded.shape == (n, 90) and np.abs(c.embedded).max() <= 4 and c.g_raw.shape == (n, 4) and np.abs(c.g_raw).max() <= 2
    assert c.raw.shape == (n, 4) and c.g_embedded.shape == (n, 90) and len(c.grads) == 24
    assert [g.shape for g in c.grads] == [shape for _, shape in orc.param_shapes()]
    live = c.g_raw.any(-1)
    assert live[-1]
    if n >= 192:      # a whole dead 64-row tile, and a tile whose only live row is its last
        assert not live[64:128].any() and not live[128:191].any() and live[191]
    if n >= 64:
        assert 0.1 <= 1 - np.concatenate([live[:64], live[192:]]).mean() <= 0.5      # "about 30 %" outside the forced tiles
    assert np.array_equal(c.g_embedded[~live], np.zeros_like(c.g_embedded[~live]))
    assert c.shift == 4 - 2 and np.abs(c.g_raw).max() * 2.0 ** c.shift == 8      # max |g_raw| = 2 -> [8, 16)
    assert c.stats["max activation"] <= 255 and c.stats["max |dz|"] * 2.0 ** c.shift <= 2048 and c.stats["max sum |terms|"] < 2.0 ** 24
    print(f"EXACT GRID n {n} seed {seed}: {c.stats}")


def test_the_launch_shift_is_the_headers():
    """max |g_raw| = m 2^e with 0.5 <= m < 1 -> s = 4 - e: the scaled maximum lies in [8, 16)."""
    for absmax, s in ((2.0, 2), (1.0, 3), (1.5, 3), (0.75, 4), (2.0 ** 41, -38), (2.0 ** -39, 42)):
        assert C.launch_shift(absmax) == s and 8 <= absmax * 2.0 ** s < 16
