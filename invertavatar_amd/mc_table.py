"""Marching-cubes case table, derived from first principles (no hand-typed table).

Cube conventions shared by the NumPy path (geometry.py), the HIP kernels (csrc/geometry.hip, through the generated
csrc/mc_tables.h) and the tests:

- corner ``c`` (0..7) sits at offset ``(c & 1, (c >> 1) & 1, (c >> 2) & 1)`` from the cell's lower corner (x, y, z);
- edge ``e`` (0..11) runs along axis ``a = e // 4`` from the corner whose other two bits (lower axis first) are ``e % 4``;
  it is the lattice edge of axis ``a`` owned by that corner's lattice point;
- case index ``sum(inside[c] << c)``, a corner being inside iff its value is above the level.

Construction (``generate``):

1. on each of the six cube faces the crossing edges are joined into segments; on an ambiguous face (the two inside corners on a
   diagonal) each inside corner is cut off on its own -- a rule that depends on the face's four corners only, so the two cells that
   share a face agree and the mesh has no cracks;
2. each segment is directed so that, seen from outside the cube, the inside corner it cuts off lies to its right; the segments
   then close into loops whose right-handed normal points away from the inside corners (toward decreasing density);
3. each loop is rotated to start at its lowest edge index and fan-triangulated; loops are emitted in the order of that edge.
"""
import numpy as np

CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], dtype=np.int64)


def edge_corners(e):
    """(start corner, end corner) of edge e."""
    a, r = divmod(e, 4)
    others = [b for b in range(3) if b != a]
    start = ((r & 1) << others[0]) | (((r >> 1) & 1) << others[1])
    return start, start | (1 << a)


EDGES = np.array([edge_corners(e) for e in range(12)], dtype=np.int64)        # [12, 2] corner ids
EDGE_AXIS = np.arange(12) // 4
EDGE_OFFSET = CORNERS[EDGES[:, 0]]                                              # [12, 3] owner offset from the cell's corner 0


def _edge_mid(e):
    s, t = EDGES[e]
    return 0.5 * (CORNERS[s] + CORNERS[t])


def faces():
    """The six faces as (axis, side, corners in cyclic order, outward normal)."""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for side in (0, 1):
            cyc = []
            for ub, uc in ((0, 0), (1, 0), (1, 1), (0, 1)):
                cyc.append((side << a) | (ub << b) | (uc << c))
            n = np.zeros(3)
            n[a] = 1.0 if side else -1.0
            out.append((a, side, cyc, n))
    return out


def _edge_between(c0, c1):
    for e in range(12):
        if set(EDGES[e]) == {c0, c1}:
            return e
    raise AssertionError((c0, c1))


def face_segments(cyc, normal, inside):
    """Directed segments (e_from, e_to) on one face; `inside` is the 8-corner mask.  Depends only on the face's corners."""
    ins = [bool(inside[c]) for c in cyc]
    cross = [(k, _edge_between(cyc[k], cyc[(k + 1) % 4])) for k in range(4) if ins[k] != ins[(k + 1) % 4]]
    pairs = []
    if len(cross) == 2:
        q = next(cyc[k] for k in range(4) if ins[k])
        pairs.append((cross[0][1], cross[1][1], q))
    elif len(cross) == 4:      # ambiguous face: each inside corner is cut off on its own
        for k in range(4):
            if ins[k]:
                e_prev = _edge_between(cyc[(k - 1) % 4], cyc[k])
                e_next = _edge_between(cyc[k], cyc[(k + 1) % 4])
                pairs.append((e_prev, e_next, cyc[k]))
    segs = []
    for e1, e2, q in pairs:
        p1, p2 = _edge_mid(e1), _edge_mid(e2)
        if np.dot(np.cross(p2 - p1, CORNERS[q] - p1), normal) > 0:
            e1, e2 = e2, e1
        segs.append((e1, e2))
    return segs


def case_loops(case):
    """Closed, outward-oriented loops of edge ids of one case, each starting at its lowest edge, ordered by that edge."""
    inside = [(case >> c) & 1 for c in range(8)]
    nxt = {}
    for _, _, cyc, n in faces():
        for e1, e2 in face_segments(cyc, n, inside):
            assert e1 not in nxt, (case, e1)
            nxt[e1] = e2
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        loops.append(loop)
    return loops


def generate():
    """(tri_count uint8 [256], tri_edges int8 [256, 3 * max_tris] padded with -1, max_tris)."""
    tris = []
    for case in range(256):
        t = []
        for loop in case_loops(case):
            for i in range(1, len(loop) - 1):
                t.append((loop[0], loop[i], loop[i + 1]))
        tris.append(t)
    max_tris = max(len(t) for t in tris)
    count = np.array([len(t) for t in tris], dtype=np.uint8)
    edges = np.full((256, 3 * max_tris), -1, dtype=np.int8)
    for case, t in enumerate(tris):
        if t:
            edges[case, :3 * len(t)] = np.array(t, dtype=np.int8).reshape(-1)
    return count, edges, max_tris


_CACHE = None


def tables():
    global _CACHE
    if _CACHE is None:
        _CACHE = generate()
    return _CACHE


def header_text():
    """Text of csrc/mc_tables.h."""
    count, edges, max_tris = generate()
    lines = ['// GENERATED by tools/gen_mc_tables.py from invertavatar_amd/mc_table.py -- do not edit.',
             '// Marching-cubes case table: corner c at (c & 1, (c >> 1) & 1, (c >> 2) & 1); edge e along axis e / 4 from the corner',
             '// whose other two bits (lower axis first) are e % 4; triangles wound so that normals point toward decreasing density.',
             '#pragma once', '', f'#define IA_MC_MAX_TRIS {max_tris}', '',
             '#ifndef IA_MC_TABLE_QUALIFIER', '#define IA_MC_TABLE_QUALIFIER static const', '#endif', '',
             'IA_MC_TABLE_QUALIFIER unsigned char ia_mc_tri_count[256] = {']
    for r in range(0, 256, 32):
        lines.append('    ' + ', '.join(str(int(v)) for v in count[r:r + 32]) + ',')
    lines += ['};', '', 'IA_MC_TABLE_QUALIFIER signed char ia_mc_tri_edges[256][3 * IA_MC_MAX_TRIS] = {']
    for case in range(256):
        lines.append('    {' + ', '.join(str(int(v)) for v in edges[case]) + '},')
    lines += ['};', '']
    return '\n'.join(lines)
