"""Ground truth for closest hits and shadow verdicts: float64 Moeller-Trumbore over EVERY world-space triangle of a scene, no tree, no
oracle (this module imports nothing from oracle/ and calls nothing of it).  TEST INFRASTRUCTURE ONLY; docs/TRACE_GROUND_TRUTH.md.

    world_triangles(fs)                      every OBJ_INSTANCE expanded: float64 [T, 3, 3] with (objid, tri_id) labels and the W2L 3x3
    closest(tris, org, dir, t_min, t_max, rule)   the winner per ray, a DECIDED flag and a candidate set
    visible(tris, org, dir, dist, rule)           scene::hitLight's opaque verdict for a punctual light, and a decided flag
    ray_sets(tris, seed)                     the five seeded ray sets of a scene

Two rules.  "world" measures t along the unit world direction: geometry.  "local" is the reference's (instance::hit re-normalises
the instance-local direction and compares the local t with the world t_max and with other instances' t): t_local = t_world *
|W2L_3x3 dir|, and selection, t_min and t_max all live in that unit.  Under rigid matrices the two agree.

BORDER / TIE / DEGENERATE sort rays into classes, they are no tolerance on a kernel: a ray is DECIDED when float64 leaves no doubt
about the answer -- one triangle at the front (or bit-equal copies of one: Triangles.klass), hit well inside (m = min(u, v, 1 - u - v)
>= BORDER), well inside (t_min, t_max), not a sliver seen edge-on, steady under the reference's perturbed box test (PERTURB below),
nothing else within TIE of it.  On a decided ray a walk has to give exactly that answer.  On the others it has to give a member of the
candidate set: every triangle with m > -BORDER that is not behind the first ROBUST hit by more than TIE (the first robust hit, not
the first hit: a winner on its own border may flip to a miss, and then the answer is whatever lies behind it), and "miss" when no
robust hit exists.

What t_max means in the reference: Traverse<Closest> prunes BOXES with t_max and never compares a triangle's t with it
(threaded_bvh_traverser.h; scene::hitLight reads `isect.t > distToLight` for that reason).  A walk may therefore report a true hit
beyond t_max, whenever a box on the way to it still overlaps the range.  `canonical` reads such a report as hitLight does -- a miss
-- after `pairs` has confirmed in float64 that the reported triangle is hit at the reported t."""
import numpy as np

from aten_amd import layout as L

BORDER = 1e-4
TIE = 1e-4
DEGENERATE = 1e-6
# The reference's box test runs on `dir + 1e-6` per component (math/aabb.h:62-86, restated in orc_core.h and device/traverse.hpp): the
# boxes are met by a ray up to sqrt(3) 1e-6 rad off the one the triangles are tested with -- sqrt(3) 1e-6 t to the side at distance t,
# and that divided by the sine of the angle between ray and triangle along the triangle's plane.  A hit is STEADY when the perturbed ray
# still meets the triangle (then it meets every box around it): the hit point is further from the triangle's edges (m times the
# smallest altitude) than twice that shift -- in world space for the top layer's boxes, and in the instance's space, where the walk
# perturbs the re-normalised local direction, for the boxes below.  A hit that is not steady is no ROBUST hit, whatever its
# barycentrics: the walk may lose it with a box around it (a ray that skims a box face over a short chord far from its origin).
PERTURB = 2.0 * np.sqrt(3.0) * 1e-6
EPS = 1e-9              # AT_MATH_EPSILON
FLOOR = 0.05            # neither outcome may fall under this share of a ray set
UNDECIDED_CAP = 0.03    # at most this share of a set may be undecided
FLT_MAX = float(np.finfo(np.float32).max)
T_FLOOR = 1e-3          # see compare
_CHUNK = 3_000_000      # ray x triangle pairs per step


class Triangles:
    """pos float64 [T, 3, 3]; objid, tri_id int64 [T] (the labels a walk reports); inst int64 [T] -> w2l float64 [I, 3, 3]."""

    def __init__(self, pos, objid, tri_id, inst, w2l):
        self.pos, self.objid, self.tri_id, self.inst, self.w2l = pos, objid, tri_id, inst, w2l
        self.centre = pos.reshape(-1, 3).mean(0)        # (everything is computed about it: the triple products cancel less)
        v0 = pos[:, 0] - self.centre
        self.e1, self.e2 = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
        self.n = np.cross(self.e1, self.e2)
        self.c0 = (v0 * self.n).sum(-1)
        self.e2xv0 = np.cross(self.e2, v0)
        self.e1xv0 = np.cross(self.e1, v0)
        self.edge = np.linalg.norm(self.e1, axis=1) * np.linalg.norm(self.e2, axis=1)
        self.nlen = np.maximum(np.linalg.norm(self.n, axis=1), 1e-300)
        longest = lambda a, b: np.maximum(np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)), np.linalg.norm(b - a, axis=1))
        self.h_w = self.nlen / np.maximum(longest(self.e1, self.e2), 1e-300)       # the smallest altitude, world
        W = w2l[inst]
        e1l, e2l = np.einsum("tij,tj->ti", W, self.e1), np.einsum("tij,tj->ti", W, self.e2)
        self.h_l = np.linalg.norm(np.cross(e1l, e2l), axis=1) / np.maximum(longest(e1l, e2l), 1e-300)     # ... in the instance's space
        self.nlen_l = np.linalg.norm(np.einsum("tji,tj->ti", np.linalg.inv(w2l)[inst], self.n), axis=1)  # |L2W^T n|
        self.bmin, self.bmax = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
        key = objid * (1 << 32) + tri_id
        self._order = np.argsort(key)
        self._keys = key[self._order]
        assert len(np.unique(key)) == len(key)
        # triangles whose world vertices are bit-equal (two instances of a mesh under the same matrix) form one class: which copy a
        # walk reports is a matter of its order, and no tie that makes a ray undecided
        _, self.klass = np.unique(pos.reshape(len(pos), 9), axis=0, return_inverse=True)
        self.klass = self.klass.reshape(-1)

    def __len__(self):
        return len(self.pos)

    def index_of(self, objid, tri_id):
        """Row of the triangle a walk names (objid, tri_id); -1 where the scene has no such triangle."""
        key = np.asarray(objid, np.int64) * (1 << 32) + np.asarray(tri_id, np.int64)
        at = np.clip(np.searchsorted(self._keys, key), 0, len(self._keys) - 1)
        return np.where(self._keys[at] == key, self._order[at], -1)


def world_triangles(fs, vtx_pos=None):
    """Every OBJ_INSTANCE of a FlatScene expanded to world space in float64.  vtx_pos: the vertices to use instead of the scene's own
    (float32 [V, >= 3]: a skinned mesh as downloaded from the device)."""
    a = fs.arrays
    objs = a["objects"]
    if (objs["type"] == L.OBJ_SPHERE).any():
        raise ValueError("brute_force: the scene holds sphere objects; only triangle scenes are expanded")
    vp = np.asarray(a["vtx_pos"] if vtx_pos is None else vtx_pos)[:, :3].astype(np.float64)
    idx = a["triangles"]["idx"]
    pos, objid, tri_id, inst, w2l = [], [], [], [], []
    for oid, o in enumerate(objs):
        if int(o["type"]) != L.OBJ_INSTANCE:
            continue
        po = objs[int(o["object_id"])]
        assert int(po["type"]) == L.OBJ_POLYGONS
        t0, tn = int(po["triangle_id"]), int(po["triangle_num"])
        v = vp[idx[t0:t0 + tn].reshape(-1)]
        mid = int(o["mtx_id"])
        W = np.eye(3)
        if mid >= 0:
            M = a["matrices"][mid].astype(np.float64)
            W = a["matrices"][mid + 1][:3, :3].astype(np.float64)
            v = v @ M[:3, :3].T + M[:3, 3]
        pos.append(v.reshape(tn, 3, 3)); objid.append(np.full(tn, oid)); tri_id.append(np.arange(t0, t0 + tn))
        inst.append(np.full(tn, len(w2l))); w2l.append(W)
    return Triangles(np.concatenate(pos), np.concatenate(objid).astype(np.int64), np.concatenate(tri_id).astype(np.int64),
                     np.concatenate(inst).astype(np.int64), np.stack(w2l))


def _unit(d):
    d = np.asarray(d, np.float64).reshape(-1, 3)
    return d / np.linalg.norm(d, axis=1)[:, None]


def _scale(tris, d, rule):
    """[R, I]: what multiplies a world t to give the rule's t, per instance."""
    if rule == "world":
        return np.ones((len(d), len(tris.w2l)))
    if rule != "local":
        raise ValueError("rule is 'world' or 'local'")
    return np.linalg.norm(np.einsum("ijk,rk->rij", tris.w2l, d), axis=-1)


def _chunks(tris, n):
    step = max(1, _CHUNK // max(1, len(tris)))
    for s in range(0, n, step):
        yield slice(s, min(n, s + step))


def _solve(tris, o, d, scale, local):
    """Moeller-Trumbore of rays (o about tris.centre, unit d) against every triangle, as five [R, 3] x [3, T] products:
    (t in the rule's unit, u, v, m, sliver measure |det| / (|e1| |e2| |d|), steady: see PERTURB), each [R, T].  local: _scale(.., 'local')."""
    dn = d @ tris.n.T                                   # det = e1 . (d x e2) = -d . n
    q = np.cross(o, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = -1.0 / dn
        t = (o @ tris.n.T - tris.c0[None, :]) * inv
        u = (q @ tris.e2.T - d @ tris.e2xv0.T) * inv
        v = (d @ tris.e1xv0.T - q @ tris.e1.T) * inv
        ts = t * scale[:, tris.inst]
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)
    ok = np.isfinite(ts) & np.isfinite(m)
    m = np.where(ok, m, -np.inf)
    ts = np.where(ok, ts, np.inf)
    with np.errstate(invalid="ignore"):
        dn = np.abs(dn)
        sl = local[:, tris.inst]
        # P t / sin < m h, world and local: sin_w = |d.n| / |n|, sin_l = |d.n| / (s |L2W^T n|), t_l = s t_w
        steady = (PERTURB * np.abs(t) * tris.nlen[None, :] < m * tris.h_w[None, :] * dn) \
            & (PERTURB * np.abs(t) * sl * sl * tris.nlen_l[None, :] < m * tris.h_l[None, :] * dn)
    return ts, u, v, m, dn / np.maximum(tris.edge, 1e-300)[None, :], steady


class Closest:
    """Per ray: hit, objid, tri_id (-1 on a miss), tindex (row in Triangles), t (rule's unit; inf on a miss), a, b, decided, miss_ok;
    the candidate triangles of UNDECIDED rays as pairs (cand_ray, cand_tri)."""

    def in_candidates(self, tris, objid, tri_id):
        """[R] bool: the answer (objid < 0 = a miss) is a member of the ray's candidate set (decided rays: the one answer)."""
        objid = np.asarray(objid, np.int64); tri_id = np.asarray(tri_id, np.int64)
        miss = objid < 0
        ti = tris.index_of(np.where(miss, 0, objid), np.where(miss, 0, tri_id))
        T = len(tris) + 1
        have = np.unique(self.cand_ray * T + self.cand_tri)
        pair = np.arange(len(objid)) * T + ti
        at = np.clip(np.searchsorted(have, pair), 0, max(len(have) - 1, 0))
        listed = (have[at] == pair) if len(have) else np.zeros(len(objid), bool)
        und = np.where(miss, self.miss_ok, listed & (ti >= 0))
        dec = np.where(miss, ~self.hit, self.hit & (ti >= 0) & (tris.klass[ti] == tris.klass[self.tindex]))
        return np.where(self.decided, dec, und)


def closest(tris, org, dir, t_min=EPS, t_max=FLT_MAX, rule="world"):
    """The closest hit of every ray over all triangles; t_max may be one value or one per ray.  See the module docstring."""
    o = np.asarray(org, np.float64).reshape(-1, 3) - tris.centre
    d = _unit(dir)
    R = len(o)
    tmax = np.broadcast_to(np.asarray(t_max, np.float64), (R,))
    tmin = float(t_min)
    scale = _scale(tris, d, rule)
    local = scale if rule == "local" else _scale(tris, d, "local")
    out = Closest()
    out.hit = np.zeros(R, bool); out.tindex = np.full(R, -1, np.int64); out.t = np.full(R, np.inf)
    out.a = np.zeros(R); out.b = np.zeros(R); out.decided = np.zeros(R, bool); out.miss_ok = np.zeros(R, bool)
    cr, ct = [], []
    for s in _chunks(tris, R):
        ts, u, v, m, sliver, steady = _solve(tris, o[s], d[s], scale[s], local[s])
        hi = tmax[s][:, None]
        accept = (m >= 0) & (ts > tmin) & (ts <= hi)
        loose = (ts > tmin * (1 - TIE)) & (ts <= hi * (1 + TIE))
        robust = (m >= BORDER) & (ts > tmin * (1 + TIE)) & (ts < hi * (1 - TIE)) & (sliver >= DEGENERATE) & steady
        tsa = np.where(accept, ts, np.inf)
        win = np.argmin(tsa, axis=1)
        rows = np.arange(len(win))
        t_best = tsa[rows, win]
        hit = np.isfinite(t_best)
        t_rb = np.where(robust, ts, np.inf).min(axis=1)
        near = (m > -BORDER) & loose & (ts <= (t_best * (1 + TIE))[:, None])
        others = (near & (tris.klass[None, :] != tris.klass[win][:, None])).any(axis=1)
        decided = np.where(hit, robust[rows, win] & ~others, ~near.any(axis=1))
        cand = (m > -BORDER) & loose & (ts <= (t_rb * (1 + TIE))[:, None]) & ~decided[:, None]
        r_, t_ = np.nonzero(cand)
        cr.append(r_ + s.start); ct.append(t_)
        out.hit[s] = hit
        out.tindex[s] = np.where(hit, win, -1)
        out.t[s] = t_best
        out.a[s] = np.where(hit, u[rows, win], 0.0); out.b[s] = np.where(hit, v[rows, win], 0.0)
        out.decided[s] = decided
        out.miss_ok[s] = ~np.isfinite(t_rb)
    out.cand_ray, out.cand_tri = np.concatenate(cr), np.concatenate(ct)
    out.objid = np.where(out.hit, tris.objid[out.tindex], -1)
    out.tri_id = np.where(out.hit, tris.tri_id[out.tindex], -1)
    return out


def pairs(tris, org, dir, tindex, rule="world"):
    """(t, u, v) in float64 of ray k against triangle tindex[k] alone."""
    o = np.asarray(org, np.float64).reshape(-1, 3) - tris.centre
    d = _unit(dir)
    e1, e2, v0 = tris.e1[tindex], tris.e2[tindex], tris.pos[tindex, 0] - tris.centre
    r = o - v0
    p = np.cross(d, e2); q = np.cross(r, e1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (p * e1).sum(-1)
        t, u, v = (q * e2).sum(-1) * inv, (p * r).sum(-1) * inv, (q * d).sum(-1) * inv
    return t * _scale(tris, d, rule)[np.arange(len(o)), tris.inst[tindex]], u, v


def canonical(tris, org, dir, hits, t_max, rule):
    """A walk's INTERSECTION records read as scene::hitLight reads them: (objid, tri_id, beyond_ok).  A hit reported beyond its t_max
    becomes a miss; beyond_ok [R] is False where float64 does not confirm that report -- the named triangle exists and is hit
    (m > -BORDER) within TIE of the reported t."""
    objid = hits["objid"].astype(np.int64); tri_id = hits["tri_id"].astype(np.int64)
    tmax = np.broadcast_to(np.asarray(t_max, np.float64), objid.shape)
    beyond = (objid >= 0) & (hits["t"].astype(np.float64) > tmax)
    ok = np.ones(len(objid), bool)
    k = np.flatnonzero(beyond)
    if len(k):
        ti = tris.index_of(objid[k], tri_id[k])
        t, u, v = pairs(tris, np.asarray(org)[k], np.asarray(dir)[k], np.maximum(ti, 0), rule)
        m = np.minimum(np.minimum(u, v), 1 - u - v)
        ok[k] = (ti >= 0) & (m > -BORDER) & (np.abs(t - hits["t"][k]) <= TIE * np.abs(t))
    return np.where(beyond, -1, objid), np.where(beyond, -1, tri_id), ok


def any_order(tris, rays, hits):
    """What EVERY order of the reference's walk respects, also where a matrix enlarges (|W2L d| < 1) and the walk's answer is neither
    rule (it prunes the top layer's WORLD boxes with a t_max held in an instance's smaller LOCAL unit, so it depends on which instance
    it met first).  For rays without a t_max, [R] bool: the reported hit X is real (float64 hits that triangle, m > -BORDER, at the
    reported local t within TIE), and no robust hit Y with a smaller local t exists that the walk cannot have skipped: Y in X's own
    instance (one unit inside an instance), or Y at a WORLD distance <= t_local(X) (every box around Y is entered before the t_max that
    X leaves).  A reported miss allows no robust hit at all.  Under matrices that do not enlarge this is rule "local" itself."""
    o = rays.org.astype(np.float64) - tris.centre
    d = _unit(rays.dir)
    scale = local = _scale(tris, d, "local")
    ok = np.zeros(len(rays), bool)
    for s in _chunks(tris, len(rays)):
        ts, u, v, m, sliver, steady = _solve(tris, o[s], d[s], scale[s], local[s])
        tw = ts / scale[s][:, tris.inst]
        robust = (m >= BORDER) & (ts > EPS * (1 + TIE)) & (sliver >= DEGENERATE) & steady
        objid, tri_id = hits["objid"][s].astype(np.int64), hits["tri_id"][s].astype(np.int64)
        miss = objid < 0
        ti = tris.index_of(np.where(miss, 0, objid), np.where(miss, 0, tri_id))
        at = np.maximum(ti, 0)
        rows = np.arange(len(at))
        tx = np.where(miss, np.inf, ts[rows, at])
        with np.errstate(invalid="ignore"):
            real = miss | ((ti >= 0) & (m[rows, at] > -BORDER) & (np.abs(tx - hits["t"][s]) <= TIE * np.abs(tx)))
            same = tris.inst[None, :] == tris.inst[at][:, None]
            must = robust & (ts * (1 + TIE) < tx[:, None]) & (miss[:, None] | same | (tw <= tx[:, None] * (1 - TIE)))
        ok[s] = real & ~must.any(axis=1)
    return ok


def visible(tris, org, dir, dist, rule="world"):
    """(visible, decided) per ray: scene::hitLight for a punctual light over opaque triangles -- visible iff no triangle is hit with
    t in (EPS, dist - EPS), in the rule's unit.  Decided: a robust blocker exists (m >= BORDER, t at least TIE inside both ends, no
    sliver), or nothing comes near blocking (no m > -BORDER triangle with t within TIE of the range)."""
    o = np.asarray(org, np.float64).reshape(-1, 3) - tris.centre
    d = _unit(dir)
    R = len(o)
    dist = np.broadcast_to(np.asarray(dist, np.float64), (R,))
    scale = _scale(tris, d, rule)
    local = scale if rule == "local" else _scale(tris, d, "local")
    vis = np.zeros(R, bool); dec = np.zeros(R, bool)
    for s in _chunks(tris, R):
        ts, u, v, m, sliver, steady = _solve(tris, o[s], d[s], scale[s], local[s])
        hi = (dist[s] - EPS)[:, None]
        blocked = ((m >= 0) & (ts > EPS) & (ts < hi)).any(axis=1)
        robust = ((m >= BORDER) & (ts > EPS * (1 + TIE)) & (ts < hi * (1 - TIE)) & (sliver >= DEGENERATE) & steady).any(axis=1)
        maybe = ((m > -BORDER) & (ts > EPS * (1 - TIE)) & (ts < hi * (1 + TIE))).any(axis=1)
        vis[s] = ~blocked
        dec[s] = robust | ~maybe
    return vis, dec


# ---- ray sets ---------------------------------------------------------------------------------------------------------------------
class Rays:
    """org, dir float32 [R, 3] (dir of unit length in float32), t_max float32 [R], set: the builder's name per ray."""

    def __init__(self, org, dir, t_max, name):
        self.org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
        n = len(self.org)
        d = np.asarray(dir, np.float64).reshape(-1, 3)
        zero = d == 0                                    # (keeps the sign of a zero component)
        d32 = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
        self.dir = np.ascontiguousarray(np.where(zero, d.astype(np.float32), d32))
        self.t_max = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float32), (n,)))
        self.set = np.ascontiguousarray(np.broadcast_to(np.asarray(name, "U16"), (n,)))

    def __len__(self):
        return len(self.org)

    def take(self, idx):
        return Rays(self.org[idx], self.dir[idx], self.t_max[idx], self.set[idx])

    @staticmethod
    def concat(sets):
        return Rays(*[np.concatenate([getattr(s, k) for s in sets]) for k in ("org", "dir", "t_max", "set")])

    def records(self):
        r = np.zeros(len(self), L.RAY)
        r["org"], r["dir"] = self.org, self.dir
        return r

    def groups(self):
        """Index arrays of the rays that share a t_max (a trace call takes one t_max)."""
        bits = self.t_max.view(np.uint32)
        order = np.argsort(bits, kind="stable")
        return np.split(order, np.flatnonzero(np.diff(bits[order])) + 1)


def trace(fn, rays):
    """INTERSECTION [R] of `rays` through fn(ray records, t_min, t_max) -> INTERSECTION array, one call per distinct t_max."""
    out = np.zeros(len(rays), L.INTERSECTION)
    rec = rays.records()
    for idx in rays.groups():
        out[idx] = fn(np.ascontiguousarray(rec[idx]), EPS, float(rays.t_max[idx[0]]))
    return out


def _points_on(tris, rng, n, clear=False):
    """n random interior points of random triangles, every instance drawn equally often: (points, unit normals, rows).
    clear: no point lies where another triangle overlaps its own in the same plane (a ray through such a point meets a tie whatever
    its direction): points whose normal probe is undecided are drawn again, six times at the most."""
    if clear:
        p, nrm, rows = _points_on(tris, rng, n)
        h = 1e-3 * float(np.linalg.norm(tris.bmax - tris.bmin))
        for _ in range(6):
            bad = np.flatnonzero(~closest(tris, p + nrm * h, -nrm, EPS, 2.0 * h, "world").decided)
            if len(bad) == 0:
                break
            p[bad], nrm[bad], rows[bad] = _points_on(tris, rng, len(bad))
        return p, nrm, rows
    insts = np.unique(tris.inst)
    which = insts[rng.integers(0, len(insts), n)]
    order = np.argsort(tris.inst, kind="stable")
    first = np.searchsorted(tris.inst[order], insts)
    count = np.diff(np.append(first, len(order)))
    k = np.searchsorted(insts, which)
    rows = order[first[k] + (rng.random(n) * count[k]).astype(np.int64)]
    u, v = rng.uniform(0.02, 0.96, n), rng.uniform(0.02, 0.96, n)
    flip = u + v > 0.98
    u, v = np.where(flip, 0.98 - u, u), np.where(flip, 0.98 - v, v)
    p = tris.pos[rows, 0] + u[:, None] * tris.e1[rows] + v[:, None] * tris.e2[rows]
    nrm = tris.n[rows]
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1), 1e-300)[:, None]
    return p, nrm, rows


def _sphere(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def ray_sets(tris, seed, rule="world", sizes=(1400, 1000, 640, 900, 64), box=1.0, aim=0.0, clear=False):
    """The five sets of a scene, about 4 096 rays:
      aimed     origins on a shell around the scene, four in five aimed at random interior points of random triangles (every instance
                equally often), the rest at random points of a larger shell
      inside    random origins in the scene box (edge scaled by `box` about its centre), random directions
      axis      origins in the box scaled by 1.3: axis-parallel directions whose other components are +0.0 / -0.0, and directions with
                one component +0.0 or -0.0
      surface   origins on surfaces pushed off along the normal, directions in that hemisphere; ONE t_max for the set, the 0.6 quantile
                of the set's unbounded hit distances: the shape of a secondary ray of bounded reach
      straddle  decided hits of the aimed set again with t_max = t_best (1 -+ 1e-3)
    aim: in a scene of few scattered triangles random rays hit next to nothing; this share of the inside / axis / surface rays passes
    through a random interior point of a random triangle instead (the axis rays by moving their origin).
    clear: the aimed set's targets and the surface set's origins avoid coplanar overlaps (_points_on), for a mesh that overlaps itself.
    The last two sets need the rule's own closest hits: this builder runs `closest` for them."""
    rng = np.random.default_rng(seed)
    n1, n2, n3, n4, n5 = sizes
    c = 0.5 * (tris.bmin + tris.bmax)
    half = 0.5 * (tris.bmax - tris.bmin)
    rad = float(np.linalg.norm(half))
    # 1
    o = c + _sphere(rng, n1) * (rad * rng.uniform(1.2, 2.5, n1))[:, None]
    target, _, _ = _points_on(tris, rng, n1, clear)
    stray = rng.random(n1) < 0.2
    target = np.where(stray[:, None], c + _sphere(rng, n1) * (rad * rng.uniform(0.6, 1.3, n1))[:, None], target)
    aimed = Rays(o, target - o, FLT_MAX, "aimed")
    # 2
    o = c + rng.uniform(-1, 1, (n2, 3)) * half * box
    d = _sphere(rng, n2)
    target, _, _ = _points_on(tris, rng, n2)
    d = np.where((rng.random(n2) < aim)[:, None], target - o, d)
    inside = Rays(o, d, FLT_MAX, "inside")
    # 3
    o = c + rng.uniform(-1, 1, (n3, 3)) * half * 1.3
    d = _sphere(rng, n3)
    ax = rng.integers(0, 3, n3)
    zero = np.where(rng.random(n3) < 0.5, 0.0, -0.0)
    par = np.arange(n3) % 2 == 0
    keep = np.arange(3)[None, :] == ax[:, None]
    # parallel: only component `ax` stays (sign kept, length 1); otherwise only component `ax` becomes a signed zero
    d = np.where(par[:, None], np.where(keep, np.sign(d), zero[:, None]), np.where(keep, zero[:, None], d))
    target, _, _ = _points_on(tris, rng, n3)
    back = target - (d / np.linalg.norm(d, axis=1)[:, None]) * (rad * rng.uniform(0.2, 1.0, n3))[:, None]
    o = np.where((rng.random(n3) < aim)[:, None], back, o)
    axis = Rays(o, d, FLT_MAX, "axis")
    # 4
    p, nrm, _ = _points_on(tris, rng, n4, clear)
    d = _sphere(rng, n4)
    target, _, _ = _points_on(tris, rng, n4)
    d = np.where((rng.random(n4) < aim)[:, None], target - p, d)
    nrm = np.where(((d * nrm).sum(-1) < 0)[:, None], -nrm, nrm)
    o = p + nrm * (1e-4 * rad)
    free = closest(tris, o.astype(np.float32), d, EPS, FLT_MAX, rule)
    reach = float(np.quantile(free.t[free.hit], 0.6)) if free.hit.any() else rad
    surface = Rays(o, d, np.float32(reach), "surface")
    # 5
    first = closest(tris, aimed.org, aimed.dir, EPS, FLT_MAX, rule)
    k = np.flatnonzero(first.hit & first.decided)[:n5]
    near = Rays(aimed.org[k], aimed.dir[k], (first.t[k] * (1 - 1e-3)).astype(np.float32), "straddle")
    far = Rays(aimed.org[k], aimed.dir[k], (first.t[k] * (1 + 1e-3)).astype(np.float32), "straddle")
    return Rays.concat([aimed, inside, axis, surface, near, far])


def check_sets(rays, hit, decided, what=""):
    """Per set: both outcomes hold at least FLOOR of the rays and at most UNDECIDED_CAP of them are undecided."""
    decided = np.asarray(decided, bool)
    for name in np.unique(rays.set):
        k = rays.set == name
        share, und = float(np.asarray(hit, bool)[k].mean()), float((~decided)[k].mean())
        assert FLOOR <= share <= 1 - FLOOR, "%s, set %s: %.3f of %d rays hit" % (what, name, share, int(k.sum()))
        assert und <= UNDECIDED_CAP, "%s, set %s: %.4f of %d rays undecided" % (what, name, und, int(k.sum()))


def compare(tris, rays, want, hits, rule, what=""):
    """A walk's hits against `want` (closest(...) of the same rays): every decided ray's object, triangle and hit-or-miss, every
    undecided ray's membership of its candidate set, every beyond-t_max report confirmed.  Returns (max relative |t - t64|, max
    |a - a64|, max |b - b64|) over the rays whose triangle agrees (0 where none does); "relative" to max(t64, T_FLOOR x the
    scene's diagonal): a hit at t = 1e-5 on the neighbouring triangle is off by the origin's float32 rounding, which its own t does not
    scale.  Raises AssertionError with the first cases."""
    objid, tri_id, beyond_ok = canonical(tris, rays.org, rays.dir, hits, rays.t_max, rule)
    ok = want.in_candidates(tris, objid, tri_id) & beyond_ok
    if not ok.all():
        bad = np.flatnonzero(~ok)
        lines = ["%s: %d of %d rays differ from float64 (%d of them decided)" % (what, len(bad), len(rays), int(want.decided[bad].sum()))]
        for i in bad[:10]:
            lines.append("  #%d [%s] org=%r dir=%r t_max=%r: got obj %d tri %d t %r; float64 obj %d tri %d t %r a %.6f b %.6f decided %d"
                         % (i, rays.set[i], rays.org[i].tolist(), rays.dir[i].tolist(), float(rays.t_max[i]), hits["objid"][i],
                            hits["tri_id"][i], float(hits["t"][i]), want.objid[i], want.tri_id[i], want.t[i], want.a[i], want.b[i], want.decided[i]))
        raise AssertionError("\n".join(lines))
    same = want.hit & (objid == want.objid) & (tri_id == want.tri_id)
    if not same.any():
        return 0.0, 0.0, 0.0
    floor = T_FLOOR * float(np.linalg.norm(tris.bmax - tris.bmin))
    return (float((np.abs(hits["t"][same] - want.t[same]) / np.maximum(want.t[same], floor)).max()),
            float(np.abs(hits["a"][same] - want.a[same]).max()), float(np.abs(hits["b"][same] - want.b[same]).max()))


def shadow_set(tris, light_pos, seed, n=2048, beyond=0.0):
    """(org, dir, dist) float32 of n shadow rays towards a point light; dir is the unnormalised vector to the light (the shadow job
    normalises it); dist is the distance to the light times a step of (0.35, 0.6, 0.85, 1.0).
    Origins: on surfaces, pushed off along the normal to the light's side (a closed hall: the blockers are its other walls and
    columns).  beyond: in a scene of a few small meshes such a ray is blocked, if at all, by its own mesh within a fraction of a unit,
    and neither the step nor the unit of t matters; this share of the origins lies BEYOND a random surface point as the light sees
    it, at 1.25 to 3 times its distance -- the blocker then sits 0.2 to 0.67 of the way from the origin to the light, on both sides
    of the stepped range's end -- and the rest lie anywhere in the scene's bounding sphere."""
    rng = np.random.default_rng(seed)
    light = np.asarray(light_pos, np.float64)[None, :]
    rad = float(np.linalg.norm(0.5 * (tris.bmax - tris.bmin)))
    p, nrm, _ = _points_on(tris, rng, n)
    nrm = np.where((((light - p) * nrm).sum(-1) < 0)[:, None], -nrm, nrm)
    o = p + nrm * (1e-4 * rad)
    if beyond > 0.0:
        far = light + (p - light) * rng.uniform(1.25, 3.0, n)[:, None]
        free = 0.5 * (tris.bmin + tris.bmax) + _sphere(rng, n) * (rad * rng.random(n) ** (1.0 / 3.0))[:, None]
        o = np.where((rng.random(n) < beyond)[:, None], far, free)
    o = o.astype(np.float32)
    d = (light - o).astype(np.float32)
    full = np.linalg.norm(d.astype(np.float64), axis=1)
    dist = (full * np.array([0.35, 0.6, 0.85, 1.0])[np.arange(n) % 4]).astype(np.float32)
    return o, d, dist


def check_verdicts(vis, decided, what=""):
    share, und = float(np.asarray(vis, bool).mean()), float((~np.asarray(decided, bool)).mean())
    assert FLOOR <= share <= 1 - FLOOR, "%s: %.3f of %d shadow rays see the light" % (what, share, len(vis))
    assert und <= UNDECIDED_CAP, "%s: %.4f of %d shadow rays undecided" % (what, und, len(vis))


# ---- the recorded bounds (profiles/parity_brute_force.jsonl) ----------------------------------------------------------------------
def records_path():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "parity_brute_force.jsonl")


def read_records():
    import json
    with open(records_path()) as f:
        return [json.loads(line) for line in f if line.strip()]


MARGIN = 4.0        # the device's leaf test performs the oracle's operations on the same triangle; only the instance entry differs in form


def float_bounds(case_name):
    """(t relative, a absolute, b absolute) a device walk is held to on `case_name`: MARGIN times what the ORACLE was measured to
    differ from float64 on that case's rays (tests/test_brute_force_cpu.py records it).  A case without a record is an error."""
    mine = [r for r in read_records() if r.get("record") == "float_bound" and r["case"] == case_name]
    if not mine:
        raise KeyError("profiles/parity_brute_force.jsonl has no float bound for %r" % (case_name,))
    return tuple(MARGIN * max(r[k] for r in mine) for k in ("t_rel", "a_abs", "b_abs"))
