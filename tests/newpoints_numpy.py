"""numpy restatement of the per-match half of
LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:283-368) as
orbx_triangulate_matches defines it, and of the neighbour loop around it.

Every float operation is a numpy float32 operation and every place where
OpenCV 2.4 accumulates in double is a float64 sum in order (DESIGN.md section
4).  The null vector of A comes from np.linalg.svd in float64, rounded once --
or from the caller (`v4`), which makes the gates independent of the
linear-algebra library: the golden fixture and the GPU tests feed recorded /
device null vectors and compare bytes.

Also here: the scene builder of the tests (3-D points seen by KF1 and n
neighbours, descriptors and FeatureVectors for the vocabulary-node search)
and the replay of the loop with the oracle's SearchForTriangulation.
"""
import ctypes
from pathlib import Path

import numpy as np

import orb_slam_amd as ox

f32, f64 = np.float32, np.float64
NLEVELS = 8
CAM = np.array([500.0, 500.0, 320.0, 240.0], f32)


# ---------------------------------------------------------------------------
# arithmetic
# ---------------------------------------------------------------------------
def fmaf(a, b, c):
    """fma(a, b, c) in float32, exactly: the product of two floats is exact in
    float64, the sum is rounded to odd there (TwoSum gives the error term),
    and 53 >= 24 + 2 bits make the final rounding the single one."""
    p = f64(a) * f64(b)
    c = f64(c)
    s = p + c
    if not np.isfinite(s):
        return f32(s)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0 and (np.array(s).view(np.uint64) & 1) == 0:
        s = np.nextafter(s, f64(np.inf) if err > 0 else f64(-np.inf))
    return f32(s)


def level_tables(nlevels=NLEVELS, scale=1.2):
    """mvScaleFactors and mvLevelSigma2 as Frame builds them in float."""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale)))
    sf = np.array(sf, f32)
    return sf, (sf * sf).astype(f32)


def make_geom(R, t, cam=CAM, nlevels=NLEVELS):
    """The dict Context.triangulate_matches takes: float32 pose, the camera
    centre Ow = -Rwc tcw, and the level tables."""
    Rcw = np.asarray(R, f64).astype(f32)
    tcw = np.asarray(t, f64).astype(f32)
    sf, s2 = level_tables(nlevels)
    return dict(Rcw=Rcw, tcw=tcw, Ow=(-(Rcw.astype(f64).T @ tcw.astype(f64))).astype(f32), cam=np.asarray(cam, f32),
                scale_factors=sf, level_sigma2=s2, nlevels=nlevels)


def _dot3(a, b):
    d = f64(a[0]) * f64(b[0])
    d = d + f64(a[1]) * f64(b[1])
    d = d + f64(a[2]) * f64(b[2])
    return d


def _cam_coord(g, r, x):
    return f32(_dot3(g["Rcw"][r], x) + f64(g["tcw"][r]))


def _ray(g, xn):
    R = g["Rcw"]
    return np.array([f32(_dot3((R[0, i], R[1, i], R[2, i]), xn)) for i in range(3)], f32)


def _norm3(x):
    return np.sqrt(_dot3(x, x))


def _xn(g, kp):
    fx, fy, cx, cy = g["cam"]
    return np.array([(kp["x"] - cx) * (f32(1.0) / fx), (kp["y"] - cy) * (f32(1.0) / fy), f32(1.0)], f32)


def build_A(g1, g2, kp1, kp2):
    """A.row(0) = xn1(0) * Tcw1.row(2) - Tcw1.row(0), ... (:303-307): a rounded
    multiply, then a rounded subtract."""
    A = np.zeros((4, 4), f32)
    for half, (g, kp) in enumerate(((g1, kp1), (g2, kp2))):
        T = np.concatenate([g["Rcw"], g["tcw"].reshape(3, 1)], 1).astype(f32)
        xn = _xn(g, kp)
        A[2 * half] = xn[0] * T[2] - T[0]
        A[2 * half + 1] = xn[1] * T[2] - T[1]
    return A


def null_vector(A):
    """The right singular vector of the smallest singular value, float64 from
    the float entries, rounded once; and (s3 - s4) / s1, which bounds how far
    two accurate solves can disagree."""
    _, s, vt = np.linalg.svd(A.astype(f64))
    return vt[3].astype(f32), (s[2] - s[3]) / s[0]


def _reproj_rejects(g, kp, x, z, contract):
    fx, fy, cx, cy = g["cam"]
    xc, yc = _cam_coord(g, 0, x), _cam_coord(g, 1, x)
    invz = f32(f64(1.0) / f64(z))
    if contract:
        u, v = fmaf(fx * xc, invz, cx), fmaf(fy * yc, invz, cy)
    else:
        u, v = fx * xc * invz + cx, fy * yc * invz + cy
    ex, ey = u - kp["x"], v - kp["y"]
    e2 = fmaf(ex, ex, ey * ey) if contract else ex * ex + ey * ey
    return bool(f64(e2) > f64(5.991) * f64(g["level_sigma2"][kp["octave"]]))


def gates(g1, g2, kp1, kp2, v4=None, contract=0):
    """One match: (status, x3D or None, v4 or None, gap or None); the status
    table is orbx.h's.  v4: the null vector to use (None: null_vector)."""
    with np.errstate(all="ignore"):
        xn1, xn2 = _xn(g1, kp1), _xn(g2, kp2)
        ray1, ray2 = _ray(g1, xn1), _ray(g2, xn2)
        cosv = f32(_dot3(ray1, ray2) / (_norm3(ray1) * _norm3(ray2)))
        if cosv < 0 or f64(cosv) > f64(0.9998):
            return 2, None, None, None
        gap = None
        if v4 is None:
            v4, gap = null_vector(build_A(g1, g2, kp1, kp2))
        v4 = np.asarray(v4, f32)
        if v4[3] == 0:
            return 3, None, v4, gap
        inv = f32(f64(1.0) / f64(v4[3]))
        x = np.array([v4[0] * inv, v4[1] * inv, v4[2] * inv], f32)
        z1 = _cam_coord(g1, 2, x)
        if z1 <= 0:
            return 4, None, v4, gap
        z2 = _cam_coord(g2, 2, x)
        if z2 <= 0:
            return 5, None, v4, gap
        if _reproj_rejects(g1, kp1, x, z1, contract):
            return 6, None, v4, gap
        if _reproj_rejects(g2, kp2, x, z2, contract):
            return 7, None, v4, gap
        dist1 = f32(_norm3((x - g1["Ow"]).astype(f32)))
        dist2 = f32(_norm3((x - g2["Ow"]).astype(f32)))
        if dist1 == 0 or dist2 == 0:
            return 8, None, v4, gap
        ratio_dist = dist1 / dist2
        ratio_octave = g1["scale_factors"][kp1["octave"]] / g2["scale_factors"][kp2["octave"]]
        ratio_factor = f32(1.5) * g1["scale_factors"][1]
        if ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor:
            return 9, None, v4, gap
        return 1, x, v4, gap


def triangulate(keys1, g1, keys2, g2, matches12, v4=None, contract=0):
    """orbx_triangulate_matches for one neighbour: status (n1), xyz (n1 x 3,
    zero where no point), v4 (n1 x 4, zero where the solve did not run), gap
    (n1, nan where null_vector did not run) and n_created."""
    n1 = len(keys1)
    out = dict(status=np.zeros(n1, np.uint8), xyz=np.zeros((n1, 3), f32), v4=np.zeros((n1, 4), f32),
               gap=np.full(n1, np.nan))
    for i in range(n1):
        j = int(matches12[i])
        if j < 0:
            continue
        st, x, v, gap = gates(g1, g2, keys1[i], keys2[j], None if v4 is None else v4[i], contract)
        out["status"][i] = st
        if x is not None:
            out["xyz"][i] = x
        if v is not None:
            out["v4"][i] = v
        if gap is not None:
            out["gap"][i] = gap
    out["n_created"] = int(np.count_nonzero(out["status"] == 1))
    return out


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def _rot(w):
    from bow_data import _rot as rot
    return rot(np.asarray(w, f64))


def make_keys(xy, octave, angle=None):
    k = np.zeros(len(xy), ox.KEYPOINT)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["response"], k["class_id"] = 31.0, 10.0, -1
    k["octave"] = octave
    if angle is not None:
        k["angle"] = angle
    return k


def _project(g, X):
    Xc = X @ g["Rcw"].astype(f64).T + g["tcw"].astype(f64)
    fx, fy, cx, cy = g["cam"].astype(f64)
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1), Xc[:, 2]


def compute_f12(g1, g2):
    """LocalMapping::ComputeF12: K1^-T [t12]x R12 K2^-1 (an input of the
    search; float64 here, rounded once)."""
    R1, t1, R2, t2 = (g1["Rcw"].astype(f64), g1["tcw"].astype(f64), g2["Rcw"].astype(f64), g2["tcw"].astype(f64))
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])

    def K(g):
        fx, fy, cx, cy = g["cam"].astype(f64)
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    return (np.linalg.inv(K(g1)).T @ tx @ R12 @ np.linalg.inv(K(g2))).astype(f32).reshape(-1)


# neighbour poses: sideways, sideways + rotation, forward + sideways
_MOTIONS = [((0.0, 0.02, 0.0), (-0.35, 0.02, 0.01)), ((0.01, -0.04, 0.01), (0.5, -0.03, 0.05)),
            ((0.0, 0.03, -0.01), (-0.25, 0.05, -1.2))]


def scene(seed, n1, n, noise=0.6, dup_frac=0.15, far_frac=0.08, bad_octave=0.1, wrong_frac=0.12, outlier_frac=0.1,
          n_nodes=24, mp_probs=(0.88, 0.08, 0.04)):
    """KF1 at a small random pose and n neighbours see a cloud 2-9 m away
    (far_frac of it at 150-400 m: no parallax).  Per neighbour the true
    matches (`truth`, with wrong_frac of them pointing at another point's
    feature, outlier_frac displaced by several pixels and bad_octave given an
    unrelated octave) exercise the gates; descriptors (a few flipped bits),
    orientations and vocabulary nodes let SearchForTriangulation find them.
    The last dup_frac * n1 KF1 keypoints are second detections of earlier
    ones -- same point, same node, nearly the same descriptor -- without a
    feature of their own in the neighbours: they match only where the first
    detection does not claim the candidate, which is what the chained loop
    changes."""
    rng = np.random.default_rng(seed)
    g1 = make_geom(_rot(rng.normal(0, 0.02, 3)), rng.normal(0, 0.05, 3))
    nd = int(dup_frac * n1)
    nb = n1 - nd
    uv = np.stack([rng.uniform(20, 620, nb), rng.uniform(20, 460, nb)], 1)
    z = rng.uniform(2.0, 9.0, nb)
    far = rng.random(nb) < far_frac
    z[far] = rng.uniform(150.0, 400.0, int(far.sum()))
    fx, fy, cx, cy = CAM.astype(f64)
    Xc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    X = (Xc - g1["tcw"].astype(f64)) @ g1["Rcw"].astype(f64)      # world
    src = rng.choice(nb, nd, replace=False) if nd else np.zeros(0, int)
    X = np.concatenate([X, X[src]])
    uv1, _ = _project(g1, X)
    uv1 += rng.normal(0, noise * 0.5, uv1.shape)
    oct1 = rng.integers(0, 5, n1)
    oct1[nb:] = oct1[src]
    pool = np.sort(rng.choice(100000, n_nodes, replace=False))
    node1 = pool[rng.integers(0, n_nodes, n1)]
    node1[nb:] = node1[src]
    desc1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    flips = (rng.random((nd, 256)) < 0.02).astype(np.uint8)
    desc1[nb:] = desc1[src] ^ np.packbits(flips, axis=1, bitorder="little")
    ang1 = rng.uniform(0, 360, n1).astype(f32)
    keys1 = make_keys(uv1.astype(f32), oct1, ang1)
    mp1 = rng.choice(3, n1, p=mp_probs).astype(np.uint8)
    out = dict(keys1=keys1, g1=g1, mp1=mp1, desc1=desc1, node1=node1, keys2=[], g2=[], mp2=[], desc2=[], node2=[],
               truth=[], F12=[])
    for k in range(n):
        w, t = _MOTIONS[k % len(_MOTIONS)]
        g2 = make_geom(_rot(np.asarray(w) + rng.normal(0, 0.01, 3)) @ g1["Rcw"].astype(f64),
                       np.asarray(t) * (1.0 + 0.3 * (k // len(_MOTIONS))) + g1["tcw"].astype(f64))
        seen = np.flatnonzero(rng.random(nb) < 0.75)
        uv2, z2 = _project(g2, X[seen])
        ok = (z2 > 0.2) & (uv2[:, 0] > 0) & (uv2[:, 0] < 640) & (uv2[:, 1] > 0) & (uv2[:, 1] < 480)
        seen, uv2 = seen[ok], uv2[ok]
        m = len(seen)
        uv2 = uv2 + rng.normal(0, noise * 0.5, uv2.shape)
        outl = rng.random(m) < outlier_frac
        uv2[outl] += rng.normal(0, 4.0, (int(outl.sum()), 2))
        n_extra = max(4, m // 4)
        n2 = m + n_extra
        xy2 = np.concatenate([uv2, np.stack([rng.uniform(0, 640, n_extra), rng.uniform(0, 480, n_extra)], 1)])
        oct2 = np.concatenate([oct1[seen], rng.integers(0, 8, n_extra)])
        bad = rng.random(m) < bad_octave
        oct2[:m][bad] = rng.integers(0, 8, int(bad.sum()))
        desc2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        fl = (rng.random((m, 256)) < rng.uniform(0.0, 0.08, (m, 1))).astype(np.uint8)
        desc2[:m] = desc1[seen] ^ np.packbits(fl, axis=1, bitorder="little")
        node2 = pool[rng.integers(0, n_nodes, n2)]
        node2[:m] = node1[seen]
        ang2 = rng.uniform(0, 360, n2).astype(f32)
        ang2[:m] = np.mod(ang1[seen] - 15.0 + rng.normal(0, 3, m), 360).astype(f32)
        perm = rng.permutation(n2)
        inv = np.argsort(perm)
        truth = np.full(n1, -1, np.int32)
        truth[seen] = inv[np.arange(m)]
        wrong = seen[rng.random(m) < wrong_frac]
        truth[wrong] = rng.integers(0, n2, len(wrong))
        out["keys2"].append(make_keys(xy2[perm].astype(f32), oct2[perm], ang2[perm]))
        out["g2"].append(g2)
        out["mp2"].append(rng.choice(3, n2, p=mp_probs).astype(np.uint8))
        out["desc2"].append(desc2[perm])
        out["node2"].append(node2[perm])
        out["truth"].append(truth)
        out["F12"].append(compute_f12(g1, g2))
    return out


def views(S, mp1=None):
    """(V1, [V2...], keep): orbx_bow_view structures over a scene."""
    from bow_data import make_view
    V1, a1 = make_view(S["keys1"], S["desc1"], S["mp1"] if mp1 is None else mp1, S["node1"])
    V2s, keep = [], [a1]
    for k in range(len(S["keys2"])):
        v, a = make_view(S["keys2"][k], S["desc2"][k], S["mp2"][k], S["node2"][k])
        V2s.append(v)
        keep.append(a)
    return V1, V2s, keep


def ref_search(V1, V2, F12, sigma2, check_ori=0):
    """The oracle's SearchForTriangulation (oracle/ref_bow.cpp)."""
    from oracle_lib import load
    fn = load().orbx_ref_search_for_triangulation
    fn.restype = ctypes.c_int
    out = np.zeros(V1.n, np.int32)
    n = ctypes.c_int()
    F12, sigma2 = np.ascontiguousarray(F12, f32), np.ascontiguousarray(sigma2, f32)
    assert fn(ctypes.byref(V1), ctypes.byref(V2), F12.ctypes.data_as(ctypes.c_void_p),
              sigma2.ctypes.data_as(ctypes.c_void_p), check_ori, out.ctypes.data_as(ctypes.c_void_p),
              ctypes.byref(n)) == 0
    return out, n.value


def replay(S, chain, check_ori=0, contract=0, v4s=None):
    """CreateNewMapPoints' neighbour loop: the oracle search, then the gates;
    chained, a created point marks its KF1 keypoint for the later
    neighbours.  v4s: per neighbour the null vectors to use (n1 x 4)."""
    mp1 = S["mp1"].copy()
    res = []
    for k in range(len(S["keys2"])):
        V1, V2s, keep = views(S, mp1)
        m, nm = ref_search(V1, V2s[k], S["F12"][k], S["g2"][k]["level_sigma2"], check_ori)
        r = triangulate(S["keys1"], S["g1"], S["keys2"][k], S["g2"][k], m, None if v4s is None else v4s[k], contract)
        r["matches12"], r["n_matches"] = m, nm
        if chain:
            mp1[r["status"] == 1] = 1
        res.append(r)
    return res


# ---------------------------------------------------------------------------
# the committed fixture
# ---------------------------------------------------------------------------
GATES_CASE = dict(seed=7, n1=300, n=3)      # the gates on the scene's `truth` matches
CHAIN_CASE = dict(seed=5, n1=300, n=3)      # the loop, searched


# Matches of scene(31, 300, 3)'s first neighbour whose KF2 keypoint was moved along y, by bisection between a
# created point and a reprojection reject, to where the two fp-contract modes decide differently: (i1, i2, y).
CONTRACT_EDITS = [(0, 129, 373.1242980957031), (4, 7, 105.36430358886719), (8, 112, 431.7764892578125)]


def contract_case():
    """(keys1, g1, keys2, g2, matches12) of the edited matches alone."""
    S = scene(31, 300, 3)
    keys1 = S["keys1"][[e[0] for e in CONTRACT_EDITS]].copy()
    keys2 = S["keys2"][0][[e[1] for e in CONTRACT_EDITS]].copy()
    keys2["y"] = [e[2] for e in CONTRACT_EDITS]
    return keys1, S["g1"], keys2, S["g2"][0], np.arange(len(CONTRACT_EDITS), dtype=np.int32)


def _pack_geom(name, g, out):
    for field in ("Rcw", "tcw", "Ow", "cam", "scale_factors", "level_sigma2"):
        out[f"{name}_{field}"] = g[field]


def unpack_contract(G):
    """contract_case() from the fixture's arrays."""
    def geom(name):
        g = {field: G[f"{name}_{field}"] for field in ("Rcw", "tcw", "Ow", "cam", "scale_factors", "level_sigma2")}
        g["nlevels"] = len(g["scale_factors"])
        return g
    return G["f_keys1"], geom("f_g1"), G["f_keys2"], geom("f_g2"), G["f_matches12"]


def _pack(prefix, S, out):
    for name in ("keys1", "mp1", "desc1", "node1"):
        out[prefix + name] = S[name]
    for k in range(len(S["keys2"])):
        for name in ("keys2", "mp2", "desc2", "node2", "truth", "F12"):
            out[f"{prefix}{name}_{k}"] = S[name][k]
    for tag, gs in (("g1", [S["g1"]]), ("g2", S["g2"])):
        for k, g in enumerate(gs):
            for name in ("Rcw", "tcw", "Ow", "cam", "scale_factors", "level_sigma2"):
                out[f"{prefix}{tag}_{k}_{name}"] = g[name]


def unpack(G, prefix, n):
    """A scene dict from the fixture's arrays."""
    def geom(tag, k):
        g = {name: G[f"{prefix}{tag}_{k}_{name}"] for name in ("Rcw", "tcw", "Ow", "cam", "scale_factors",
                                                                 "level_sigma2")}
        g["nlevels"] = len(g["scale_factors"])
        return g
    S = {name: G[prefix + name] for name in ("keys1", "mp1", "desc1", "node1")}
    S["g1"] = geom("g1", 0)
    S["g2"] = [geom("g2", k) for k in range(n)]
    for name in ("keys2", "mp2", "desc2", "node2", "truth", "F12"):
        S[name] = [G[f"{prefix}{name}_{k}"] for k in range(n)]
    return S


def golden_arrays():
    out = {}
    S = scene(**GATES_CASE)
    _pack("g_", S, out)
    for k in range(GATES_CASE["n"]):
        for c in (0, 1):
            r = triangulate(S["keys1"], S["g1"], S["keys2"][k], S["g2"][k], S["truth"][k], contract=c)
            out[f"g_status{c}_{k}"], out[f"g_xyz{c}_{k}"] = r["status"], r["xyz"]
        out[f"g_v4_{k}"] = r["v4"]
    S = scene(**CHAIN_CASE)
    _pack("c_", S, out)
    for chain in (0, 1):
        for k, r in enumerate(replay(S, chain)):
            for name in ("matches12", "status", "xyz", "v4"):
                out[f"c_{name}{chain}_{k}"] = r[name]
    keys1, g1, keys2, g2, m = contract_case()
    out["f_keys1"], out["f_keys2"], out["f_matches12"] = keys1, keys2, m
    _pack_geom("f_g1", g1, out)
    _pack_geom("f_g2", g2, out)
    for c in (0, 1):
        r = triangulate(keys1, g1, keys2, g2, m, contract=c)
        out[f"f_status{c}"], out[f"f_xyz{c}"] = r["status"], r["xyz"]
    out["f_v4"] = r["v4"]
    assert np.all(out["f_status0"] != out["f_status1"])
    return out


def write_golden(path):
    np.savez_compressed(path, **golden_arrays())


if __name__ == "__main__":
    write_golden(Path(__file__).resolve().parent / "golden" / "new_points.npz")
