#!/usr/bin/env python3
"""Generates pl-nerf_amd/csrc/mc_table.h, the marching-cubes case table of csrc/mesh.hip and tests/mesh_model.py.

    python tools/gen_mc_table.py            # prints the header
    python tools/gen_mc_table.py --write    # rewrites pl-nerf_amd/csrc/mc_table.h

Nothing is typed from memory: every row is derived from the cube's geometry by the rule below, and tests/test_mesh_table_host.py
holds the committed header to this script's output byte for byte and the rows to the invariants that make a mesh closed.

The cube.  Corner i sits at (i & 1, (i >> 1) & 1, (i >> 2) & 1) = (dx, dy, dz) from the cell's lattice point; bit i of a cell's
STATE is set when corner i is inside (f >= iso).  Edge e = 4 a + u + 2 v runs along axis a from the corner whose offsets along
the two OTHER axes (in ascending order) are (u, v); that corner is the edge's owning lattice point, which is how csrc/mesh.hip
finds the vertex on it.  An edge crosses when exactly one of its ends is inside.

The rule, face by face (so that the two cells that share a face agree: it reads only the face's four corners).  The crossing
edges of a face are joined into segments: with two of them, one segment; with four (two diagonal inside corners, the ambiguous
face), each inside corner is cut off separately -- its segment joins the two face edges that meet in it.  A segment is directed
so that, seen from outside the cube, the inside corners lie to its RIGHT.  Every crossing edge then ends one segment and begins
another; following them gives closed loops, each traversed counter-clockwise seen from the outside region, so that triangle
normals (v1 - v0) x (v2 - v0) point towards decreasing field.  A loop is triangulated as a fan from its lowest-numbered edge
among those whose fan has no diagonal lying in a face of the cube (see fan()), loops in the order of their lowest edge."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pl-nerf_amd", "csrc", "mc_table.h")


def corner_offsets(i):
    return (i & 1, (i >> 1) & 1, (i >> 2) & 1)


def corner_id(off):
    return off[0] | (off[1] << 1) | (off[2] << 2)


def other_axes(a):
    return [b for b in range(3) if b != a]


def edge_id(a, off):
    """The edge along axis a through the corner offsets `off` (off[a] is ignored)."""
    b, c = other_axes(a)
    return 4 * a + off[b] + 2 * off[c]


def edge_owner(e):
    """(offsets of the edge's first corner = its owning lattice point, axis)."""
    a, k = divmod(e, 4)
    b, c = other_axes(a)
    off = [0, 0, 0]
    off[b], off[c] = k & 1, k >> 1
    return tuple(off), a


def edge_corners(e):
    off, a = edge_owner(e)
    far = list(off)
    far[a] = 1
    return corner_id(off), corner_id(far)


def edge_midpoint(e):
    off, a = edge_owner(e)
    m = [float(x) for x in off]
    m[a] = 0.5
    return m


def faces():
    """Every face as (normal axis, side, its four corners in cyclic order, its four edges: edge k joins corners k and k + 1)."""
    out = []
    for n in range(3):
        b, c = other_axes(n)
        for side in (0, 1):
            corners, offs = [], []
            for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[n], off[b], off[c] = side, u, v
                offs.append(off)
                corners.append(corner_id(off))
            edges = []
            for k in range(4):
                p, q = offs[k], offs[(k + 1) % 4]
                a = next(x for x in range(3) if p[x] != q[x])
                edges.append(edge_id(a, p))
            out.append((n, side, corners, edges))
    return out


def _cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def face_segments(state, face):
    """The directed segments (edge, edge) the rule puts on one face of a cell in `state`."""
    n, side, corners, edges = face
    inside = [(state >> c) & 1 for c in corners]
    crossing = [k for k in range(4) if inside[k] != inside[(k + 1) % 4]]
    if not crossing:
        return []
    if len(crossing) == 2:
        # one segment; any inside corner tells the side (all of them lie on one side of it)
        pairs = [(edges[crossing[0]], edges[crossing[1]], corners[inside.index(1)])]
    else:
        # the ambiguous face: corner k meets face edges k - 1 and k
        pairs = [(edges[(k - 1) % 4], edges[k], corners[k]) for k in range(4) if inside[k]]
    normal = [0.0, 0.0, 0.0]
    normal[n] = 1.0 if side else -1.0      # (towards the viewer outside the cube)
    out = []
    for e1, e2, corner in pairs:
        m1, m2 = edge_midpoint(e1), edge_midpoint(e2)
        d = [y - x for x, y in zip(m1, m2)]
        mid = [(x + y) / 2 for x, y in zip(m1, m2)]
        to_corner = [float(x) - y for x, y in zip(corner_offsets(corner), mid)]
        left = sum(x * y for x, y in zip(_cross(normal, d), to_corner))      # > 0: the inside corner is to the left
        assert left != 0.0, (state, face, e1, e2)
        out.append((e2, e1) if left > 0 else (e1, e2))
    return out


def loops(state):
    """The closed loops of crossing edges of a cell in `state`, each from its lowest edge on, in the order of those."""
    nxt = {}
    for face in faces():
        for e1, e2 in face_segments(state, face):
            assert e1 not in nxt, (state, e1)
            nxt[e1] = e2
    crossing = [e for e in range(12) if ((state >> edge_corners(e)[0]) ^ (state >> edge_corners(e)[1])) & 1]
    assert sorted(nxt) == sorted(nxt.values()) == crossing, (state, nxt, crossing)
    out, seen = [], set()
    for e in crossing:
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        assert len(loop) >= 3 and not seen & set(loop), (state, loop)
        seen |= set(loop)
        out.append(loop)
    return out


def cofacial(e1, e2):
    """Do two cube edges lie on one face?"""
    return any(e1 in edges and e2 in edges for _, _, _, edges in faces())


def fan(loop):
    """The loop as a fan from its lowest-numbered edge whose diagonals all run through the cell's interior.  A diagonal
    between two edges of one face would lie IN that face -- an ambiguous one, which the loop visits twice -- and the cell
    behind the face may draw the same diagonal: one mesh edge in four triangles.  (The lowest edge itself serves 340 of the 358
    loops; tests/test_mesh_table_host.py holds every row to the rule.)"""
    n = len(loop)
    for apex in sorted(loop):
        k = loop.index(apex)
        turned = loop[k:] + loop[:k]
        if not any(cofacial(turned[0], turned[j]) for j in range(2, n - 1)):
            return [(turned[0], turned[i], turned[i + 1]) for i in range(1, n - 1)]
    raise AssertionError(("no fan without a diagonal in a face", loop))


def triangles(state):
    return [t for loop in loops(state) for t in fan(loop)]


def table():
    return [triangles(state) for state in range(256)]


def render():
    rows = table()
    most = max(len(r) for r in rows)
    width = 3 * most
    out = [
        "// GENERATED by tools/gen_mc_table.py -- do not edit; tests/test_mesh_table_host.py compares this file with the script's output.",
        "// The marching-cubes case table of csrc/mesh.hip (and of tests/mesh_model.py): corner i of a cell sits at offsets",
        "// (i & 1, (i >> 1) & 1, (i >> 2) & 1) along (x, y, z), bit i of the state is set when that corner is inside (f >= iso);",
        "// edge e = 4 a + u + 2 v runs along axis a from the corner with offsets (u, v) along the other two axes in ascending order.",
        "// plnerf_mc_tri[state] lists the state's triangles as edge triples (counter-clockwise seen from the outside region: normals",
        "// towards decreasing field), plnerf_mc_ntri[state] how many there are (at most %d); the rest of a row is -1." % most,
        "#pragma once",
        "#ifndef PLNERF_MC_TABLE_QUALIFIER",
        "#define PLNERF_MC_TABLE_QUALIFIER",
        "#endif",
        "#define PLNERF_MC_MAX_TRI %d" % most,
        "#define PLNERF_MC_ROW %d" % width,
        "static PLNERF_MC_TABLE_QUALIFIER const unsigned char plnerf_mc_ntri[256] = {",
    ]
    for r0 in range(0, 256, 32):
        out.append("    " + ", ".join(str(len(rows[s])) for s in range(r0, r0 + 32)) + ",")
    out += ["};", "static PLNERF_MC_TABLE_QUALIFIER const signed char plnerf_mc_tri[256][PLNERF_MC_ROW] = {"]
    for s, r in enumerate(rows):
        flat = [e for t in r for e in t]
        flat += [-1] * (width - len(flat))
        out.append("    {" + ", ".join("%2d" % e for e in flat) + "},  // %3d" % s)
    out += ["};", ""]
    return "\n".join(out)


if __name__ == "__main__":
    text = render()
    if "--write" in sys.argv[1:]:
        with open(HEADER, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
