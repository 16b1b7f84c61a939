#!/usr/bin/env python3
"""Generate laenerf_amd/csrc/mc_table.inc: the marching-cubes case table of csrc/mesh.hip and laenerf_amd/mesh.py.

Cube corner c = dx + 2 dy + 4 dz (x = the field's first axis).  Edge e = 4 * axis + n, where n counts the corners whose bit
`axis` is 0 in increasing order: edge e runs from that corner along `axis`.  A corner is inside iff value > threshold.

Per case (the 8 inside bits), the polygon on each of the 6 cube faces is built from that face's edge crossings: two crossings
give one segment; four (the inside corners on one diagonal: the ambiguous face) give two segments, each cutting off one
INSIDE corner -- the inside corners are separated.  That choice depends on the face's 4 corners only, so two cubes sharing a
face put the same segments on it and the mesh is watertight.  Each segment is directed so that the surface's right-hand normal
points from inside to outside (towards lower density); the segments chain into closed loops (each crossed edge lies on two
faces: one segment enters it, one leaves), and each loop is fan-triangulated from its lowest edge id whose fan has no diagonal
between two edges of one face.  Such a diagonal could be drawn by the neighbouring cube too (two edges on an ambiguous face that
the face's segments do not join, both on one loop in each cube): that mesh edge would then lie in four triangles.  A diagonal
between two edges on no common face belongs to this cube alone.  (Every loop of every case has such an apex; the lowest edge id
itself serves in 196 of 214 loops of four or more edges.)
"""
import os

CORNER = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
EDGES = [(c, a) for a in range(3) for c in range(8) if not (c >> a) & 1]      # e -> (start corner, axis)


def edge_end(e):
    c, a = EDGES[e]
    return c | (1 << a)


def edge_mid(e):
    c, a = EDGES[e]
    p = [float(v) for v in CORNER[c]]
    p[a] += 0.5
    return p


def _sub(p, q):
    return [p[0] - q[0], p[1] - q[1], p[2] - q[2]]


def _cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def _dot(p, q):
    return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]


def faces():
    """-> [(axis, side, outward normal, corners in cyclic order, edges of the face)]"""
    out = []
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        for s in (0, 1):
            n = [0.0, 0.0, 0.0]
            n[a] = 1.0 if s else -1.0
            ring = []
            for ub, ud in ((0, 0), (1, 0), (1, 1), (0, 1)):
                ring.append((s << a) | (ub << b) | (ud << d))
            fe = [e for e in range(12) if EDGES[e][1] != a and ((EDGES[e][0] >> a) & 1) == s]
            out.append((a, s, n, ring, fe))
    return out


FACES = faces()


def case_loops(case):
    """the closed, oriented loops of crossed edge ids of one case"""
    inside = [(case >> c) & 1 for c in range(8)]
    crossed = [e for e in range(12) if inside[EDGES[e][0]] != inside[edge_end(e)]]
    nxt = {}
    for a, s, n, ring, fe in FACES:
        fc = [e for e in fe if e in crossed]
        if not fc:
            continue
        if len(fc) == 2:
            pairs = [tuple(fc)]
        else:                                              # ambiguous face: one segment around each inside corner
            assert len(fc) == 4
            pairs = []
            for c in ring:
                if inside[c]:
                    pairs.append(tuple(e for e in fc if c in (EDGES[e][0], edge_end(e))))
        for p, q in pairs:
            # the inside endpoint of p's edge lies on the segment's inside side; keep p -> q when n x (q - p) points away from it
            ci = EDGES[p][0] if inside[EDGES[p][0]] else edge_end(p)
            mp = edge_mid(p)
            m = _cross(n, _sub(edge_mid(q), mp))
            side = _dot(_sub([float(v) for v in CORNER[ci]], mp), m)
            assert side != 0
            if side > 0:
                p, q = q, p
            assert p not in nxt, (case, p)
            nxt[p] = q
    assert sorted(nxt) == crossed and sorted(nxt.values()) == crossed, case
    loops, left = [], set(crossed)
    while left:
        start = min(left)
        loop, e = [], start
        while True:
            loop.append(e)
            left.discard(e)
            e = nxt[e]
            if e == start:
                break
        loops.append(loop)                                 # starts at its lowest edge id (min of the remaining ones)
    return loops, crossed


def fan_apex(loop):
    """the lowest edge id of the loop whose fan draws no diagonal between two edges of one face"""
    faces_of = [{f for f, face in enumerate(FACES) if e in face[4]} for e in range(12)]
    for e in sorted(loop):
        r = loop.index(e)
        rot = loop[r:] + loop[:r]
        if not any(faces_of[e] & faces_of[d] for d in rot[2:-1]):
            return e
    raise AssertionError(loop)


def build():
    """-> (triangle edge triples per case, 12-bit crossing masks, MC_MAX_TRIS)"""
    tris, masks = [], []
    for case in range(256):
        loops, crossed = case_loops(case)
        t = []
        for loop in loops:
            r = loop.index(fan_apex(loop))
            loop = loop[r:] + loop[:r]
            for i in range(1, len(loop) - 1):
                t.append((loop[0], loop[i], loop[i + 1]))
        tris.append(t)
        masks.append(sum(1 << e for e in crossed))
    return tris, masks, max(len(t) for t in tris)


def render():
    tris, masks, max_tris = build()
    L = ["// GENERATED by tools/gen_mc_table.py -- do not edit.",
         "// Marching-cubes cases: corner c = dx + 2*dy + 4*dz; edge e = (MC_EDGE_CORNER[e], MC_EDGE_AXIS[e]); corner inside iff",
         "// value > threshold.  Ambiguous faces separate the inside corners; loops are oriented inside -> outside and fanned",
         "// from their lowest edge id whose fan draws no diagonal between two edges of one face.",
         "#define MC_MAX_TRIS %d" % max_tris,
         "__constant__ uint8_t MC_EDGE_CORNER[12] = {%s};" % ", ".join(str(c) for c, _ in EDGES),
         "__constant__ uint8_t MC_EDGE_AXIS[12] = {%s};" % ", ".join(str(a) for _, a in EDGES),
         "__constant__ uint16_t MC_EDGE_MASK[256] = {"]
    for r in range(0, 256, 16):
        L.append("    " + ", ".join("0x%03x" % m for m in masks[r:r + 16]) + ",")
    L.append("};")
    L.append("__constant__ uint8_t MC_TRI_COUNT[256] = {")
    for r in range(0, 256, 32):
        L.append("    " + ", ".join(str(len(t)) for t in tris[r:r + 32]) + ",")
    L.append("};")
    L.append("__constant__ int8_t MC_TRI_EDGES[256][3 * MC_MAX_TRIS] = {")
    for case, t in enumerate(tris):
        flat = [e for tri in t for e in tri] + [-1] * (3 * (max_tris - len(t)))
        L.append("    {" + ", ".join(str(e) for e in flat) + "},  // %d" % case)
    L.append("};")
    return "\n".join(L) + "\n"


OUT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "laenerf_amd", "csrc", "mc_table.inc"))


def main():
    with open(OUT, "w") as f:
        f.write(render())
    print("wrote", OUT)


if __name__ == "__main__":
    main()
