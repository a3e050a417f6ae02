"""The marching-cubes case table pl-nerf_amd/csrc/mc_table.h, without a GPU: it is tools/gen_mc_table.py's output byte for byte;
every row's loops are closed and use every crossing edge once; the two cells behind any face agree on that face's segments, in
opposite directions (the crack-free and orientation proof: 16 face states x 3 axes); complementary states use the same edges;
no fan diagonal lies in a face of the cube; and the meshes tests/mesh_model.py builds on the table are closed, oriented
surfaces (its invariants, called here because pytest collects test_*.py files only)."""
import os
import sys
from collections import Counter

import pytest

import mesh_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mc_table
    finally:
        sys.path.pop(0)
    return gen_mc_table


@pytest.fixture(scope="module")
def table():
    ntri, tri = mesh_model.load_table()
    return [[tuple(int(e) for e in tri[s, 3 * k:3 * k + 3]) for k in range(int(ntri[s]))] for s in range(256)], tri


def test_the_header_is_the_generators_output(gen):
    assert open(gen.HEADER).read() == gen.render()
    assert mesh_model.TABLE_HEADER == gen.HEADER


def test_rows_are_padded_and_as_long_as_the_generator_yields(table, gen):
    rows, tri = table
    most = max(len(r) for r in rows)
    assert most == 5 and tri.shape == (256, 3 * most)      # the row length the generator yields: 15
    for s, r in enumerate(rows):
        assert (tri[s, 3 * len(r):] == -1).all() and (tri[s, :3 * len(r)] >= 0).all() and (tri[s] < 12).all(), s
        assert r == gen.triangles(s)
    # the model's restated edge numbering is the generator's
    assert all(mesh_model.edge_owner(e) == gen.edge_owner(e) for e in range(12))


def _boundary(triangles):
    """The directed edges of a row that no opposite edge of the row cancels: the loops' segments (a fan's diagonals are used
    once in each direction)."""
    edges = Counter()
    for a, b, c in triangles:
        for e in ((a, b), (b, c), (c, a)):
            edges[e] += 1
    return Counter({e: n - edges.get((e[1], e[0]), 0) for e, n in edges.items() if n > edges.get((e[1], e[0]), 0)})


def _crossing(gen, state):
    return {e for e in range(12) if ((state >> gen.edge_corners(e)[0]) ^ (state >> gen.edge_corners(e)[1])) & 1}


def test_every_loop_is_closed_and_every_crossing_edge_is_used_once(table, gen):
    rows, _ = table
    for s, r in enumerate(rows):
        seg = _boundary(r)
        assert set(seg.values()) <= {1}, (s, seg)
        nxt = dict(seg.keys())
        assert len(nxt) == len(seg), (s, "an edge begins two segments")
        assert set(nxt) == set(nxt.values()) == _crossing(gen, s), (s, nxt)
        # following the segments closes loops of at least three edges, and a loop of n edges carries n - 2 triangles
        seen, loops = set(), 0
        for e in sorted(nxt):
            if e in seen:
                continue
            loop = [e]
            while nxt[loop[-1]] != e:
                loop.append(nxt[loop[-1]])
                assert len(loop) <= 12, s
            assert len(loop) >= 3, (s, loop)
            seen |= set(loop)
            loops += 1
        assert len(r) == len(nxt) - 2 * loops, s
        for t in r:
            assert len(set(t)) == 3, (s, t)


def _face_key(gen, face):
    """{edge of the face: (its axis, its offset along the face's remaining in-plane axis)}: the same key on either side."""
    n, side, corners, edges = face
    out = {}
    for e in edges:
        off, a = gen.edge_owner(e)
        (b,) = [x for x in range(3) if x not in (n, a)]
        out[e] = (a, off[b])
    return out


def test_cells_that_share_a_face_agree_on_it_in_opposite_directions(table, gen):
    rows, _ = table
    segments = {s: set(_boundary(r)) for s, r in enumerate(rows)}
    for n in range(3):
        low = next(f for f in gen.faces() if f[0] == n and f[1] == 0)
        high = next(f for f in gen.faces() if f[0] == n and f[1] == 1)
        klow, khigh = _face_key(gen, low), _face_key(gen, high)
        # corner k of the high face and corner k of the low face are the same lattice point seen from the two cells
        assert [gen.corner_offsets(c)[:n] + gen.corner_offsets(c)[n + 1:] for c in low[2]] == \
               [gen.corner_offsets(c)[:n] + gen.corner_offsets(c)[n + 1:] for c in high[2]]
        for face_state in range(16):
            def on(face, key, s):
                if [(s >> c) & 1 for c in face[2]] != [(face_state >> k) & 1 for k in range(4)]:
                    return None
                return frozenset((key[a], key[b]) for a, b in segments[s] if a in key and b in key)
            from_high = {on(high, khigh, s) for s in range(256)} - {None}      # the cell below the face sees its own high face
            from_low = {on(low, klow, s) for s in range(256)} - {None}
            assert len(from_high) == 1 and len(from_low) == 1, (n, face_state)      # the rule reads the face's corners only
            (h,), (l,) = from_high, from_low
            assert l == frozenset((b, a) for a, b in h), (n, face_state, h, l)
            crossing = sum(((face_state >> k) ^ (face_state >> ((k + 1) % 4))) & 1 for k in range(4))
            assert len(h) == crossing // 2


def test_complementary_states_use_the_same_edges(table):
    rows, _ = table
    for s in range(256):
        assert {e for t in rows[s] for e in t} == {e for t in rows[255 - s] for e in t}, s


def test_no_diagonal_lies_in_a_face(table, gen):
    """A triangle edge that is not a loop segment joins two cube edges of no common face: it runs through the cell's interior,
    so the neighbour cannot draw it too (which on white noise put one mesh edge into four triangles)."""
    rows, _ = table
    for s, r in enumerate(rows):
        seg = set(_boundary(r))
        for a, b, c in r:
            for e in ((a, b), (b, c), (c, a)):
                if e not in seg:
                    assert not gen.cofacial(*e), (s, e)


def test_noise_meshes_are_closed_and_oriented():
    mesh_model.check_noise_meshes_are_closed_and_oriented()


def test_sphere_is_one_closed_surface_with_outward_normals():
    mesh_model.check_sphere_is_one_closed_surface_with_outward_normals()


def test_the_fields_reach_every_state():
    mesh_model.check_the_fields_reach_every_state()
