"""Host-side logic of the use_batching ray source (no GPU): the epoch schedule of RayBank against the reference's
i_batch loop (run_plnerf.py:1238-1249), and dp.shard_batch's balanced split of a global batch of any size."""
import pytest
import torch

import abi_support as abi


@pytest.fixture(scope="module")
def built():
    """The package, with the library built first if it is absent (no GPU needed)."""
    abi.built_lib()
    import plnerf_amd
    return plnerf_amd


def _reference_walk(M, N_rand, epochs):
    """The reference loop's bookkeeping, literally: per step the rows [i_batch, i_batch + N_rand) of rays_rgb (the last
    slice of an epoch is short: numpy slicing stops at M), then `i_batch += N_rand` and a reshuffle with i_batch = 0 once
    i_batch >= M.  Yields (epoch, first row, rows) per step."""
    i_batch, epoch = 0, 0
    while epoch < epochs:
        n = len(range(M)[i_batch:i_batch + N_rand])
        yield epoch, i_batch, n
        i_batch += N_rand
        if i_batch >= M:
            epoch += 1
            i_batch = 0


@pytest.mark.parametrize("M,B", [(612, 50), (612, 51), (612, 612), (612, 700), (100, 1), (7, 3), (1024, 256),
                                 (3 * 12 * 17, 4096), (513, 128), (578, 192)])
def test_schedule_is_the_reference_i_batch_loop(built, M, B):
    images = torch.zeros(1, 1, M, 3)
    poses = torch.eye(4)[None]
    bank = built.RayBank(images, poses, [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]], [0], 0.0, 1.0, device="cpu")
    assert bank.M == M
    walk = list(_reference_walk(M, B, 3))
    assert walk[-1][0] == 2 and sum(n for _, _, n in walk) == 3 * M
    for g, want in enumerate(walk):
        assert bank.schedule(g, B) == want, (g, bank.schedule(g, B), want)
        assert built.batch_schedule(g, M, B) == want
    # stateless: any step on its own, far past the start (a resumed run), is the walk's
    S = -(-M // B)
    for g in (10 * S, 10 * S + S - 1, 123457):
        e, p0, n = bank.schedule(g, B)
        assert e == g // S and p0 == (g % S) * B and n == min(B, M - p0) and 0 < n <= B


def test_bank_from_training_views(built):
    images = torch.rand(5, 12, 17, 3)
    poses = torch.eye(4).repeat(5, 1, 1)
    bank = built.RayBank(images, poses, [[20.0, 0, 8.5], [0, 20.0, 6], [0, 0, 1]], [0, 2, 4], 0.0, 1.0, seed=3, device="cpu")
    assert bank.M == 3 * 12 * 17 and bank.poses.shape == (5, 12) and bank.views.dtype == torch.int32
    assert bank.views.tolist() == [0, 2, 4]
    t, r, c = built.RayBank.decode(torch.tensor([0, 17, 12 * 17, 2 * 12 * 17 + 5 * 17 + 16]), 12, 17)
    assert t.tolist() == [0, 0, 1, 2] and r.tolist() == [0, 1, 0, 5] and c.tolist() == [0, 0, 0, 16]
    with pytest.raises(ValueError):
        built.RayBank(images, poses, bank.K, [0, 5], 0.0, 1.0, device="cpu")
    with pytest.raises(ValueError):
        built.RayBank(images, poses, bank.K, [], 0.0, 1.0, device="cpu")


def test_step_batch_refuses_precrop(built):
    ts = built.TrainStep.__new__(built.TrainStep)
    with pytest.raises(ValueError, match="precrop"):
        ts.step_batch(None, 16, precrop=(4, 4))


@pytest.mark.parametrize("world", [1, 2, 3, 4, 7, 8])
def test_shard_batch_is_contiguous_balanced_and_covers_the_batch(built, world):
    from plnerf_amd import dp
    for n in list(range(0, 40)) + [4095, 4096, 32768, 32769]:
        parts = [dp.shard_batch(n, r, world) for r in range(world)]
        assert parts[0][0] == 0 and parts[-1][1] == n
        for (b0, e0), (b1, e1) in zip(parts, parts[1:]):
            assert e0 == b1                                    # contiguous and disjoint
        sizes = [e - b for b, e in parts]
        assert max(sizes) - min(sizes) <= 1 and sorted(sizes, reverse=True) == sizes
        for r, (b, e) in enumerate(parts):
            assert e - b == n // world + (r < n % world) and b == r * (n // world) + min(r, n % world)
        if n % world == 0:
            assert parts == [dp.shard_rays(n, r, world) for r in range(world)]
            assert parts == [(r * n // world, (r + 1) * n // world) for r in range(world)]
        if 0 < n < world:
            assert sizes.count(0) == world - n
    with pytest.raises(ValueError):
        dp.shard_batch(10, world, world)
