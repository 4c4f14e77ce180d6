"""orb_slam_amd -- MI355X-native ORB-SLAM front end and local-BA kernels.

Python view of liborbx (include/orbx.h), used by tests and bench.py.  The
product is the C ABI + HIP kernels in orb_slam_amd/csrc; the production
binding is the C++ adapter in orb_slam_amd/adapters.

There is no CPU fallback: if liborbx.so is missing or no GPU is visible, the
entry points raise.
"""
import ctypes
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("ORBX_LIBRARY", _PKG / "liborbx.so"))

ORBX_OK = 0
ERRORS = {-1: "ORBX_ERR_ARG", -2: "ORBX_ERR_HIP", -3: "ORBX_ERR_CAPACITY",
          -4: "ORBX_ERR_UNSUPPORTED", -5: "ORBX_ERR_NOMEM", -6: "ORBX_ERR_NOT_POSDEF"}

# cv::KeyPoint / orbx_keypoint (28 bytes)
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT.itemsize == 28


class OrbxError(RuntimeError):
    def __init__(self, code, where):
        super().__init__(f"{where}: {ERRORS.get(code, code)}")
        self.code = code


class FrameView(ctypes.Structure):
    _fields_ = [("keys_un", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("n", ctypes.c_int),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float),
                ("min_y", ctypes.c_float), ("max_y", ctypes.c_float),
                ("nlevels", ctypes.c_int), ("scale_factor", ctypes.c_float)]


class InitQuery(ctypes.Structure):
    """orbx_init_query (include/orbx.h)."""
    _fields_ = [("keys1", ctypes.c_void_p), ("n1", ctypes.c_int), ("keys2", ctypes.c_void_p), ("n2", ctypes.c_int),
                ("matches12", ctypes.c_void_p), ("sigma", ctypes.c_float), ("max_iter", ctypes.c_int),
                ("draws", ctypes.c_void_p),
                ("n_matches", ctypes.c_int), ("best_h", ctypes.c_int), ("best_f", ctypes.c_int),
                ("SH", ctypes.c_float), ("SF", ctypes.c_float), ("RH", ctypes.c_float),
                ("H21", ctypes.c_float * 9), ("F21", ctypes.c_float * 9),
                ("inliers_h", ctypes.c_void_p), ("inliers_f", ctypes.c_void_p), ("cap", ctypes.c_int),
                ("sets", ctypes.c_void_p), ("Hn", ctypes.c_void_p), ("Fn", ctypes.c_void_p),
                ("H21_all", ctypes.c_void_p), ("H12_all", ctypes.c_void_p), ("F21_all", ctypes.c_void_p),
                ("score_h", ctypes.c_void_p), ("score_f", ctypes.c_void_p),
                ("T1", ctypes.c_void_p), ("T2", ctypes.c_void_p)]


_INIT_TAPS = (("sets", np.int32, 8), ("Hn", np.float32, 9), ("Fn", np.float32, 9), ("H21_all", np.float32, 9),
              ("H12_all", np.float32, 9), ("F21_all", np.float32, 9), ("score_h", np.float32, 0),
              ("score_f", np.float32, 0))


def init_query(keys1, keys2, matches12, draws, sigma=1.0, max_iter=200, taps=False, cap=None):
    """An InitQuery over numpy arrays and the arrays it points to (keep both
    alive while the query is used): (query, keep)."""
    keep = {}
    q = InitQuery()
    if keys1 is not None:
        keep["keys1"] = np.ascontiguousarray(keys1, KEYPOINT)
        keep["keys2"] = np.ascontiguousarray(keys2, KEYPOINT)
        keep["matches12"] = np.ascontiguousarray(matches12, np.int32)
        keep["draws"] = np.ascontiguousarray(draws, np.int32)
        q.keys1, q.n1 = keep["keys1"].ctypes.data, len(keep["keys1"])
        q.keys2, q.n2 = keep["keys2"].ctypes.data, len(keep["keys2"])
        q.matches12, q.draws = keep["matches12"].ctypes.data, keep["draws"].ctypes.data
        if cap is None:
            cap = len(keep["keys1"])
    q.sigma, q.max_iter = sigma, max_iter
    q.cap = max(int(cap), 0)
    keep["inliers_h"], keep["inliers_f"] = np.zeros(max(q.cap, 1), np.uint8), np.zeros(max(q.cap, 1), np.uint8)
    q.inliers_h, q.inliers_f = keep["inliers_h"].ctypes.data, keep["inliers_f"].ctypes.data
    if taps:
        m = max(int(max_iter), 1)
        for name, dt, k in _INIT_TAPS:
            keep[name] = np.zeros((m, k) if k else m, dt)
            setattr(q, name, keep[name].ctypes.data)
        for name in ("T1", "T2"):
            keep[name] = np.zeros(9, np.float32)
            setattr(q, name, keep[name].ctypes.data)
    return q, keep


def init_result(q, keep, taps=False):
    """The out fields (and taps) of a filled InitQuery as a dict."""
    n = q.n_matches
    r = dict(n_matches=n, best_h=q.best_h, best_f=q.best_f, SH=np.float32(q.SH), SF=np.float32(q.SF),
             RH=np.float32(q.RH), H21=np.array(q.H21, np.float32) if q.best_h >= 0 else None,
             F21=np.array(q.F21, np.float32) if q.best_f >= 0 else None,
             inliers_h=keep["inliers_h"][:n].copy(), inliers_f=keep["inliers_f"][:n].copy())
    if taps:
        for name, _, _ in _INIT_TAPS:
            r[name] = keep[name]
        r["T1"], r["T2"] = keep["T1"], keep["T2"]
    return r


# The reference compares the float RH with the double 0.40 (src/Initializer.cc:113), which holds for RH >= 0.40f;
# orbx_dev_init_reconstruct compares floats, so the float just below 0.40f reproduces it for every RH.
RH_THRESHOLD = float(np.nextafter(np.float32(0.40), np.float32(0)))


class ReconstructQuery(ctypes.Structure):
    """orbx_reconstruct_query (include/orbx.h)."""
    _fields_ = [("keys1", ctypes.c_void_p), ("n1", ctypes.c_int), ("keys2", ctypes.c_void_p), ("n2", ctypes.c_int),
                ("matches12", ctypes.c_void_p), ("inliers", ctypes.c_void_p), ("model", ctypes.c_int),
                ("M21", ctypes.c_void_p), ("cam", ctypes.c_void_p), ("sigma", ctypes.c_float),
                ("min_parallax", ctypes.c_float), ("min_triangulated", ctypes.c_int),
                ("ok", ctypes.c_int), ("n_inliers", ctypes.c_int), ("n_hyp", ctypes.c_int), ("best", ctypes.c_int),
                ("R21", ctypes.c_float * 9), ("t21", ctypes.c_float * 3),
                ("n_good", ctypes.c_int32 * 8), ("parallax", ctypes.c_float * 8),
                ("p3d", ctypes.c_void_p), ("triangulated", ctypes.c_void_p), ("cap", ctypes.c_int),
                ("svd", ctypes.c_void_p), ("R_all", ctypes.c_void_p), ("t_all", ctypes.c_void_p),
                ("v4", ctypes.c_void_p), ("cos_parallax", ctypes.c_void_p)]


def reconstruct_query(keys1, keys2, matches12, inliers, model, M21, cam, sigma=1.0, min_parallax=1.0,
                      min_triangulated=50, taps=False, cap=None, n_max=None):
    """A ReconstructQuery over numpy arrays and the arrays it points to (keep
    both alive while the query is used): (query, keep).  keys1 None: an
    output-only query of a device-resident pair (cap keypoints, n_max matches)."""
    keep = {}
    q = ReconstructQuery()
    if keys1 is not None:
        keep["keys1"] = np.ascontiguousarray(keys1, KEYPOINT)
        keep["keys2"] = np.ascontiguousarray(keys2, KEYPOINT)
        keep["matches12"] = np.ascontiguousarray(matches12, np.int32)
        keep["inliers"] = np.ascontiguousarray(inliers, np.uint8)
        keep["M21"] = np.ascontiguousarray(M21, np.float32).reshape(-1)
        keep["cam"] = np.ascontiguousarray(cam, np.float32).reshape(-1)
        q.keys1, q.n1 = keep["keys1"].ctypes.data, len(keep["keys1"])
        q.keys2, q.n2 = keep["keys2"].ctypes.data, len(keep["keys2"])
        q.matches12, q.inliers = keep["matches12"].ctypes.data, keep["inliers"].ctypes.data
        q.M21, q.cam = keep["M21"].ctypes.data, keep["cam"].ctypes.data
        q.model = int(model)
        n_max = int(np.count_nonzero(keep["matches12"] >= 0))
        if cap is None:
            cap = len(keep["keys1"])
    q.sigma, q.min_parallax, q.min_triangulated = sigma, min_parallax, min_triangulated
    q.cap = max(int(cap), 0)
    keep["p3d"], keep["triangulated"] = np.zeros((max(q.cap, 1), 3), np.float32), np.zeros(max(q.cap, 1), np.uint8)
    q.p3d, q.triangulated = keep["p3d"].ctypes.data, keep["triangulated"].ctypes.data
    keep["n_max"] = int(n_max)
    if taps:
        for name, shape in (("svd", 21), ("R_all", (8, 9)), ("t_all", (8, 3)), ("v4", (8 * max(n_max, 1), 4)),
                            ("cos_parallax", 8 * max(n_max, 1))):
            keep[name] = np.zeros(shape, np.float32)
            setattr(q, name, keep[name].ctypes.data)
    return q, keep


def reconstruct_result(q, keep, taps=False, n1=None, n_matches=None):
    """The out fields (and taps) of a filled ReconstructQuery as a dict; v4
    and cos_parallax as (n_hyp, N, 4) and (n_hyp, N)."""
    n1 = q.n1 if n1 is None else n1
    r = dict(ok=q.ok, n_inliers=q.n_inliers, n_hyp=q.n_hyp, best=q.best,
             R21=np.array(q.R21, np.float32) if q.ok else None, t21=np.array(q.t21, np.float32) if q.ok else None,
             n_good=np.array(q.n_good, np.int32), parallax=np.array(q.parallax, np.float32),
             p3d=keep["p3d"][:n1].copy(), triangulated=keep["triangulated"][:n1].copy())
    if taps:
        N = keep["n_max"] if n_matches is None else n_matches
        r["svd"], r["R_all"], r["t_all"] = keep["svd"], keep["R_all"], keep["t_all"]
        r["v4"] = keep["v4"][:q.n_hyp * N].reshape(q.n_hyp, N, 4)
        r["cos_parallax"] = keep["cos_parallax"][:q.n_hyp * N].reshape(q.n_hyp, N)
    return r


class Sim3Query(ctypes.Structure):
    """orbx_sim3_query (include/orbx.h)."""
    _fields_ = [("keys1", ctypes.c_void_p), ("n1", ctypes.c_int), ("keys2", ctypes.c_void_p), ("n2", ctypes.c_int),
                ("matches12", ctypes.c_void_p), ("idx1", ctypes.c_void_p),
                ("pos1", ctypes.c_void_p), ("valid1", ctypes.c_void_p),
                ("pos2", ctypes.c_void_p), ("valid2", ctypes.c_void_p),
                ("T1w", ctypes.c_void_p), ("T2w", ctypes.c_void_p), ("cam1", ctypes.c_void_p), ("cam2", ctypes.c_void_p),
                ("sigma2_1", ctypes.c_void_p), ("sigma2_2", ctypes.c_void_p), ("nlevels", ctypes.c_int),
                ("probability", ctypes.c_double), ("min_inliers", ctypes.c_int), ("max_iterations", ctypes.c_int),
                ("iter_done", ctypes.c_int), ("best_inliers", ctypes.c_int), ("n_iter", ctypes.c_int),
                ("draws", ctypes.c_void_p),
                ("N", ctypes.c_int), ("ransac_max_its", ctypes.c_int), ("iters_run", ctypes.c_int),
                ("no_more", ctypes.c_int), ("found", ctypes.c_int), ("found_iter", ctypes.c_int),
                ("n_inliers", ctypes.c_int), ("T12", ctypes.c_float * 16),
                ("inliers", ctypes.c_void_p), ("cap", ctypes.c_int),
                ("best_inliers_out", ctypes.c_int), ("best_iter", ctypes.c_int),
                ("R12", ctypes.c_float * 9), ("t12", ctypes.c_float * 3), ("s12", ctypes.c_float),
                ("sets", ctypes.c_void_p), ("q", ctypes.c_void_p), ("R", ctypes.c_void_p), ("scale", ctypes.c_void_p),
                ("T12_all", ctypes.c_void_p), ("T21_all", ctypes.c_void_p), ("count", ctypes.c_void_p),
                ("x3dc1", ctypes.c_void_p), ("x3dc2", ctypes.c_void_p), ("p1im1", ctypes.c_void_p),
                ("p2im2", ctypes.c_void_p), ("max_err1", ctypes.c_void_p), ("max_err2", ctypes.c_void_p),
                ("indices1", ctypes.c_void_p)]


class Sim3Kf(ctypes.Structure):
    """orbx_sim3_kf (include/orbx.h)."""
    _fields_ = [("mp", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("Tcw", ctypes.c_void_p), ("cam", ctypes.c_void_p),
                ("sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int)]


_SIM3_ITER_TAPS = (("sets", np.int32, 3), ("q", np.float32, 4), ("R", np.float32, 9), ("scale", np.float32, 0),
                   ("T12_all", np.float32, 16), ("T21_all", np.float32, 16), ("count", np.int32, 0))
_SIM3_CORR_TAPS = (("x3dc1", np.float32, 3), ("x3dc2", np.float32, 3), ("p1im1", np.float32, 2),
                   ("p2im2", np.float32, 2), ("max_err1", np.int32, 0), ("max_err2", np.int32, 0),
                   ("indices1", np.int32, 0))
_SIM3_KF_KEYS = ("keys", "pos", "valid", "Tcw", "cam", "sigma2")


def sim3_query(kf1, kf2, matches12, draws, n_iter=None, idx1=None, probability=0.99, min_inliers=20,
               max_iterations=300, iter_done=0, best_inliers=0, taps=False, cap=None):
    """A Sim3Query over numpy arrays and the arrays it points to (keep both
    alive while the query is used): (query, keep).  kf1 / kf2: dicts of keys
    (KEYPOINT), pos (n x 3), valid (n), Tcw (4 x 4), cam (fx, fy, cx, cy) and
    sigma2 (the level table).  kf1 None: an output-only query of a
    device-resident candidate (cap keypoints)."""
    keep = {}
    q = Sim3Query()
    if kf1 is not None:
        for side, kf in (("1", kf1), ("2", kf2)):
            keep["keys" + side] = np.ascontiguousarray(kf["keys"], KEYPOINT)
            keep["pos" + side] = np.ascontiguousarray(kf["pos"], np.float32).reshape(-1, 3)
            keep["valid" + side] = np.ascontiguousarray(kf["valid"], np.uint8)
            keep["T" + side + "w"] = np.ascontiguousarray(kf["Tcw"], np.float32).reshape(-1)
            keep["cam" + side] = np.ascontiguousarray(kf["cam"], np.float32).reshape(-1)
            keep["sigma2_" + side] = np.ascontiguousarray(kf["sigma2"], np.float32).reshape(-1)
            for name in ("keys", "pos", "valid"):
                setattr(q, name + side, keep[name + side].ctypes.data)
            for name in ("T" + side + "w", "cam" + side, "sigma2_" + side):
                setattr(q, name, keep[name].ctypes.data)
        q.n1, q.n2 = len(keep["keys1"]), len(keep["keys2"])
        q.nlevels = min(len(keep["sigma2_1"]), len(keep["sigma2_2"]))
        keep["matches12"] = np.ascontiguousarray(matches12, np.int32)
        keep["draws"] = np.ascontiguousarray(draws, np.int32)
        q.matches12, q.draws = keep["matches12"].ctypes.data, keep["draws"].ctypes.data
        if idx1 is not None:
            keep["idx1"] = np.ascontiguousarray(idx1, np.int32)
            q.idx1 = keep["idx1"].ctypes.data
        if n_iter is None:
            n_iter = keep["draws"].size // 3
        if cap is None:
            cap = q.n1
    q.probability, q.min_inliers, q.max_iterations = probability, min_inliers, max_iterations
    q.iter_done, q.best_inliers, q.n_iter = iter_done, best_inliers, int(n_iter)
    q.cap = max(int(cap), 0)
    keep["inliers"] = np.zeros(max(q.cap, 1), np.uint8)
    q.inliers = keep["inliers"].ctypes.data
    if taps:
        m = max(int(n_iter), 1)
        for name, dt, k in _SIM3_ITER_TAPS:
            keep[name] = np.zeros((m, k) if k else m, dt)
            setattr(q, name, keep[name].ctypes.data)
        for name, dt, k in _SIM3_CORR_TAPS:
            keep[name] = np.zeros((max(q.cap, 1), k) if k else max(q.cap, 1), dt)
            setattr(q, name, keep[name].ctypes.data)
    return q, keep


def sim3_result(q, keep, taps=False, n1=None):
    """The out fields (and taps) of a filled Sim3Query as a dict."""
    n1 = q.n1 if n1 is None else n1
    r = dict(N=q.N, ransac_max_its=q.ransac_max_its, iters_run=q.iters_run, no_more=q.no_more, found=q.found,
             found_iter=q.found_iter, n_inliers=q.n_inliers, best_inliers_out=q.best_inliers_out, best_iter=q.best_iter,
             T12=np.array(q.T12, np.float32) if q.found else None,
             R12=np.array(q.R12, np.float32) if q.best_iter >= 0 else None,
             t12=np.array(q.t12, np.float32) if q.best_iter >= 0 else None,
             s12=np.float32(q.s12) if q.best_iter >= 0 else None, inliers=keep["inliers"][:n1].copy())
    if taps:
        for name, _, _ in _SIM3_ITER_TAPS:
            r[name] = keep[name]
        for name, _, _ in _SIM3_CORR_TAPS:
            r[name] = keep[name][:q.N]
    return r


class Sim3OptQuery(ctypes.Structure):
    """orbx_sim3_opt_query (include/orbx.h)."""
    _fields_ = [("keys1", ctypes.c_void_p), ("n1", ctypes.c_int), ("keys2", ctypes.c_void_p), ("n2", ctypes.c_int),
                ("matches12", ctypes.c_void_p),
                ("pos1", ctypes.c_void_p), ("valid1", ctypes.c_void_p),
                ("pos2", ctypes.c_void_p), ("valid2", ctypes.c_void_p),
                ("T1w", ctypes.c_void_p), ("T2w", ctypes.c_void_p), ("cam1", ctypes.c_void_p), ("cam2", ctypes.c_void_p),
                ("inv_sigma2_1", ctypes.c_void_p), ("sigma2_2", ctypes.c_void_p), ("nlevels", ctypes.c_int),
                ("R12", ctypes.c_float * 9), ("t12", ctypes.c_float * 3), ("s12", ctypes.c_float),
                ("th2", ctypes.c_float),
                ("n_in", ctypes.c_int), ("n_corr", ctypes.c_int), ("n_bad", ctypes.c_int),
                ("returned_early", ctypes.c_int),
                ("q12", ctypes.c_double * 4), ("t12d", ctypes.c_double * 3), ("s12d", ctypes.c_double),
                ("iterations", ctypes.c_int * 2), ("trials", ctypes.c_int * 2), ("not_posdef", ctypes.c_int * 2),
                ("cap", ctypes.c_int), ("corr_index", ctypes.c_void_p),
                ("x3dc1", ctypes.c_void_p), ("x3dc2", ctypes.c_void_p),
                ("edge_err", ctypes.c_void_p), ("edge_J", ctypes.c_void_p), ("edge_chi2", ctypes.c_void_p),
                ("n_lm", ctypes.c_int),
                ("it_est", ctypes.c_void_p), ("it_chi2", ctypes.c_void_p), ("it_H", ctypes.c_void_p),
                ("it_b", ctypes.c_void_p), ("it_lambda", ctypes.c_void_p), ("it_trials", ctypes.c_void_p),
                ("it_dx", ctypes.c_void_p), ("check_est", ctypes.c_void_p)]


SIM3_OPT_MAX_LM, SIM3_OPT_MAX_TRIALS = 15, 10
_SIM3OPT_CORR_TAPS = (("corr_index", np.int32, 0), ("x3dc1", np.float32, 3), ("x3dc2", np.float32, 3),
                      ("edge_err", np.float64, 4), ("edge_J", np.float64, 28))
_SIM3OPT_ITER_TAPS = (("it_est", np.float64, 8), ("it_chi2", np.float64, 0), ("it_H", np.float64, 28),
                      ("it_b", np.float64, 7), ("it_lambda", np.float64, 0), ("it_trials", np.int32, 0),
                      ("it_dx", np.float64, (SIM3_OPT_MAX_TRIALS, 7)))


def sim3_opt_query(kf1, kf2, matches12, R12, t12, s12, th2=10.0, taps=False, cap=None):
    """A Sim3OptQuery over numpy arrays and the arrays it points to (keep both
    alive while the query is used): (query, keep).  kf1 / kf2: dicts of keys
    (KEYPOINT), pos (n x 3), valid (n), Tcw (4 x 4), cam (fx, fy, cx, cy);
    kf1 also inv_sigma2 (its mvInvLevelSigma2), kf2 sigma2 (its mvLevelSigma2
    -- what the reference reads for e21).  matches12 is copied: the copy is the
    in / out array.  kf1 None: the query of a device-resident candidate
    (matches12 holds cap entries)."""
    keep = {}
    q = Sim3OptQuery()
    if kf1 is not None:
        for side, kf in (("1", kf1), ("2", kf2)):
            keep["keys" + side] = np.ascontiguousarray(kf["keys"], KEYPOINT)
            keep["pos" + side] = np.ascontiguousarray(kf["pos"], np.float32).reshape(-1, 3)
            keep["valid" + side] = np.ascontiguousarray(kf["valid"], np.uint8)
            keep["T" + side + "w"] = np.ascontiguousarray(kf["Tcw"], np.float32).reshape(-1)
            keep["cam" + side] = np.ascontiguousarray(kf["cam"], np.float32).reshape(-1)
            for name in ("keys", "pos", "valid"):
                setattr(q, name + side, keep[name + side].ctypes.data)
            for name in ("T" + side + "w", "cam" + side):
                setattr(q, name, keep[name].ctypes.data)
        keep["inv_sigma2_1"] = np.ascontiguousarray(kf1["inv_sigma2"], np.float32).reshape(-1)
        keep["sigma2_2"] = np.ascontiguousarray(kf2["sigma2"], np.float32).reshape(-1)
        q.inv_sigma2_1, q.sigma2_2 = keep["inv_sigma2_1"].ctypes.data, keep["sigma2_2"].ctypes.data
        q.n1, q.n2 = len(keep["keys1"]), len(keep["keys2"])
        q.nlevels = min(len(keep["inv_sigma2_1"]), len(keep["sigma2_2"]))
    keep["matches12"] = np.array(matches12, np.int32).reshape(-1)
    q.matches12 = keep["matches12"].ctypes.data
    q.R12[:] = np.asarray(R12, np.float32).reshape(9).tolist()
    q.t12[:] = np.asarray(t12, np.float32).reshape(3).tolist()
    q.s12, q.th2 = float(s12), float(th2)
    if cap is None:
        cap = len(keep["matches12"])
    q.cap = max(int(cap), 0)
    if taps:
        m = max(q.cap, 1)
        for name, dt, k in _SIM3OPT_CORR_TAPS:
            keep[name] = np.zeros((m, k) if k else m, dt)
            setattr(q, name, keep[name].ctypes.data)
        keep["edge_chi2"] = np.full((2, m, 2), np.nan)
        q.edge_chi2 = keep["edge_chi2"].ctypes.data
        for name, dt, k in _SIM3OPT_ITER_TAPS:
            shape = (SIM3_OPT_MAX_LM,) + (k if isinstance(k, tuple) else ((k,) if k else ()))
            keep[name] = np.zeros(shape, dt)
            setattr(q, name, keep[name].ctypes.data)
        keep["check_est"] = np.zeros((2, 8))
        q.check_est = keep["check_est"].ctypes.data
    return q, keep


def sim3_opt_result(q, keep, taps=False):
    """The out fields (and taps) of a filled Sim3OptQuery as a dict: matches12
    (out), n_in (OptimizeSim3's return value), n_corr, n_bad, returned_early,
    q12 / t12d / s12d and the float R12 / t12 / s12 (None on the early exit,
    where the reference leaves g2oS12 alone), iterations / trials / not_posdef
    per round."""
    done = not q.returned_early
    r = dict(matches12=keep["matches12"], n_in=q.n_in, n_corr=q.n_corr, n_bad=q.n_bad,
             returned_early=q.returned_early,
             q12=np.array(q.q12) if done else None, t12d=np.array(q.t12d) if done else None,
             s12d=float(q.s12d) if done else None,
             R12=np.array(q.R12, np.float32).reshape(3, 3) if done else None,
             t12=np.array(q.t12, np.float32) if done else None, s12=np.float32(q.s12) if done else None,
             iterations=list(q.iterations), trials=list(q.trials), not_posdef=list(q.not_posdef))
    if taps:
        r["n_lm"] = q.n_lm
        for name, _, _ in _SIM3OPT_CORR_TAPS:
            r[name] = keep[name][:q.n_corr]
        r["edge_chi2"] = keep["edge_chi2"][:, :q.n_corr]
        for name, _, _ in _SIM3OPT_ITER_TAPS:
            r[name] = keep[name][:q.n_lm]
        r["check_est"] = keep["check_est"]
    return r


class EssGraphQuery(ctypes.Structure):
    """orbx_essgraph_query (include/orbx.h)."""
    _fields_ = [("kfs", ctypes.c_void_p), ("n_kf", ctypes.c_int), ("loop_kf", ctypes.c_int), ("cur_kf", ctypes.c_int),
                ("edges", ctypes.c_void_p), ("n_edges", ctypes.c_int),
                ("pos", ctypes.c_void_p), ("ref_kf", ctypes.c_void_p), ("n_points", ctypes.c_int),
                ("Tcw_out", ctypes.c_void_p), ("pos_out", ctypes.c_void_p), ("est_out", ctypes.c_void_p),
                ("iterations", ctypes.c_int), ("trials", ctypes.c_int), ("not_posdef", ctypes.c_int),
                ("chi2_first", ctypes.c_double), ("chi2_last", ctypes.c_double), ("lambda_last", ctypes.c_double),
                ("n_free", ctypes.c_int), ("n_blocks", ctypes.c_longlong), ("max_row_blocks", ctypes.c_int),
                ("edge_meas", ctypes.c_void_p), ("edge_err", ctypes.c_void_p), ("edge_J", ctypes.c_void_p),
                ("it_chi2", ctypes.c_void_p), ("it_lambda", ctypes.c_void_p), ("it_trials", ctypes.c_void_p),
                ("it_est", ctypes.c_void_p), ("it_b", ctypes.c_void_p), ("it_dx", ctypes.c_void_p),
                ("it_Hdiag", ctypes.c_void_p)]


# orbx_essgraph_kf (192 bytes) and orbx_essgraph_edge (12 bytes)
ESSGRAPH_KF = np.dtype([("id", "<i8"), ("Tcw", "<f4", 12), ("has_corrected", "<i4"), ("has_noncorrected", "<i4"),
                        ("corrected", "<f8", 8), ("noncorrected", "<f8", 8)])
ESSGRAPH_EDGE = np.dtype({"names": ["i", "j", "kind"], "formats": ["<i4", "<i4", "u1"], "offsets": [0, 4, 8],
                          "itemsize": 12})
assert ESSGRAPH_KF.itemsize == 192
ESSGRAPH_MAX_LM = 20


def essgraph_arrays(ids, Tcw, edges, corrected=None, noncorrected=None):
    """The keyframe and edge arrays of an essential graph: ids (n), Tcw (n x 12,
    R row-major then t, or n x 4 x 4 / n x 3 x 4), edges (m x 3: i, j, kind),
    corrected / noncorrected: {keyframe index: Sim3 (x, y, z, w, tx, ty, tz, s)}."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    n = len(ids)
    T = np.asarray(Tcw, np.float32)
    if T.ndim == 3:
        T = np.concatenate([T[:, :3, :3].reshape(n, 9), T[:, :3, 3]], 1)
    kfs = np.zeros(n, ESSGRAPH_KF)
    kfs["id"], kfs["Tcw"] = ids, T.reshape(n, 12)
    for name, table in (("corrected", corrected), ("noncorrected", noncorrected)):
        for k, v in (table or {}).items():
            kfs["has_" + name][k] = 1
            kfs[name][k] = np.asarray(v, np.float64)
    e = np.asarray(edges, np.int64).reshape(-1, 3)
    ed = np.zeros(len(e), ESSGRAPH_EDGE)
    ed["i"], ed["j"], ed["kind"] = e[:, 0], e[:, 1], e[:, 2]
    return kfs, ed


def essgraph_query(kfs, edges, loop_kf, cur_kf, pos=None, ref_kf=None, taps=False):
    """An EssGraphQuery over numpy arrays and the arrays it points to (keep both
    alive while the query is used): (query, keep).  kfs / edges: ESSGRAPH_KF and
    ESSGRAPH_EDGE arrays (essgraph_arrays); pos (n x 3) / ref_kf (n): the map
    points and the index of each one's reference keyframe (-1: skipped).  The
    outputs start as NaN (pos_out as a copy of pos), so what a call does not
    write is visible."""
    keep = dict(kfs=np.ascontiguousarray(kfs, ESSGRAPH_KF), edges=np.ascontiguousarray(edges, ESSGRAPH_EDGE))
    q = EssGraphQuery()
    n, m = len(keep["kfs"]), len(keep["edges"])
    q.kfs, q.n_kf, q.loop_kf, q.cur_kf = keep["kfs"].ctypes.data, n, int(loop_kf), int(cur_kf)
    q.edges, q.n_edges = keep["edges"].ctypes.data, m
    # copies: `keep` owns what the query points to, so writing into it never reaches the caller's arrays
    keep["pos"] = np.array(pos if pos is not None else np.zeros((0, 3)), np.float32, order="C").reshape(-1, 3)
    keep["ref_kf"] = np.array(ref_kf if ref_kf is not None else np.zeros(0), np.int32, order="C").reshape(-1)
    npts = len(keep["pos"])
    q.pos, q.ref_kf, q.n_points = keep["pos"].ctypes.data, keep["ref_kf"].ctypes.data, npts
    keep["Tcw_out"] = np.full((n, 12), np.nan, np.float32)
    keep["pos_out"] = keep["pos"].copy()
    keep["est_out"] = np.full((n, 8), np.nan)
    q.Tcw_out, q.pos_out, q.est_out = keep["Tcw_out"].ctypes.data, keep["pos_out"].ctypes.data, keep["est_out"].ctypes.data
    if taps:
        L = ESSGRAPH_MAX_LM
        shapes = dict(edge_meas=(m, 8), edge_err=(m, 7), edge_J=(m, 98), it_chi2=(L,), it_lambda=(L,),
                      it_est=(L, n, 8), it_b=(L, 7 * n), it_dx=(L, 7 * n), it_Hdiag=(L, n * 28))
        for name, shape in shapes.items():
            keep[name] = np.full(shape, np.nan)
            setattr(q, name, keep[name].ctypes.data)
        keep["it_trials"] = np.zeros(L, np.int32)
        q.it_trials = keep["it_trials"].ctypes.data
    return q, keep


def essgraph_result(q, keep, taps=False):
    """The out fields (and taps) of a filled EssGraphQuery as a dict.  The
    per-iteration taps are cut to the iterations run and to n_free."""
    r = dict(Tcw=keep["Tcw_out"], pos=keep["pos_out"], est=keep["est_out"], iterations=q.iterations, trials=q.trials,
             not_posdef=q.not_posdef, chi2_first=q.chi2_first, chi2_last=q.chi2_last, lambda_last=q.lambda_last,
             n_free=q.n_free, n_blocks=q.n_blocks, max_row_blocks=q.max_row_blocks)
    if taps:
        it, nf, n = q.iterations, q.n_free, q.n_kf
        for name in ("edge_meas", "edge_err", "edge_J"):
            r[name] = keep[name]
        for name in ("it_chi2", "it_lambda", "it_trials"):
            r[name] = keep[name][:it]
        r["it_est"] = keep["it_est"].reshape(-1)[:it * n * 8].reshape(it, n, 8)
        r["it_b"] = keep["it_b"].reshape(-1)[:it * nf * 7].reshape(it, nf * 7)
        r["it_dx"] = keep["it_dx"].reshape(-1)[:it * nf * 7].reshape(it, nf * 7)
        r["it_Hdiag"] = keep["it_Hdiag"].reshape(-1)[:it * nf * 28].reshape(it, nf, 28)
    return r


def essgraph_plan(ids, fixed, edges):
    """orbx_essgraph_plan (host only, no GPU): the envelope of the block
    Cholesky over the free vertices in id order.  edges: an ESSGRAPH_EDGE
    array or m x 3 integers.  A dict of free_index (n_kf), first (n_free),
    row_off (n_free + 1), n_free, n_blocks, max_row_blocks."""
    ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
    if not (isinstance(edges, np.ndarray) and edges.dtype == ESSGRAPH_EDGE):
        e = np.asarray(edges, np.int64).reshape(-1, 3)
        edges = np.zeros(len(e), ESSGRAPH_EDGE)
        edges["i"], edges["j"], edges["kind"] = e[:, 0], e[:, 1], e[:, 2]
    edges = np.ascontiguousarray(edges)
    n = len(ids)
    free_index, first, row_off = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64)
    nf, nb, mx = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int()
    _check(lib().orbx_essgraph_plan(n, _ptr(ids), int(fixed), len(edges), _ptr(edges), _ptr(free_index), _ptr(first),
                                    _ptr(row_off), ctypes.byref(nf), ctypes.byref(nb), ctypes.byref(mx)),
           "orbx_essgraph_plan")
    return dict(free_index=free_index, first=first[:nf.value], row_off=row_off[:nf.value + 1], n_free=nf.value,
                n_blocks=nb.value, max_row_blocks=mx.value)


class PnpQuery(ctypes.Structure):
    """orbx_pnp_query (include/orbx.h)."""
    _fields_ = [("keys", ctypes.c_void_p), ("n", ctypes.c_int), ("pos", ctypes.c_void_p), ("valid", ctypes.c_void_p),
                ("cam", ctypes.c_void_p), ("sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int),
                ("probability", ctypes.c_double), ("min_inliers", ctypes.c_int), ("max_iterations", ctypes.c_int),
                ("min_set", ctypes.c_int), ("epsilon", ctypes.c_float), ("th2", ctypes.c_float),
                ("iter_done", ctypes.c_int), ("best_inliers", ctypes.c_int), ("best_mask", ctypes.c_void_p),
                ("best_Tcw", ctypes.c_float * 16),
                ("n_iter", ctypes.c_int), ("n_draws", ctypes.c_int), ("draws", ctypes.c_void_p),
                ("N", ctypes.c_int), ("ransac_min_inliers", ctypes.c_int), ("ransac_max_its", ctypes.c_int),
                ("iters_run", ctypes.c_int), ("no_more", ctypes.c_int), ("found", ctypes.c_int),
                ("found_iter", ctypes.c_int), ("n_inliers", ctypes.c_int), ("refined", ctypes.c_int),
                ("Tcw", ctypes.c_float * 16), ("inliers", ctypes.c_void_p), ("cap", ctypes.c_int),
                ("n_records", ctypes.c_int), ("best_slot", ctypes.c_int),
                ("p2d", ctypes.c_void_p), ("p3d", ctypes.c_void_p), ("max_err", ctypes.c_void_p),
                ("kp_index", ctypes.c_void_p),
                ("sets", ctypes.c_void_p), ("rec", ctypes.c_void_p), ("count", ctypes.c_void_p),
                ("refit_rec", ctypes.c_void_p), ("refit_count", ctypes.c_void_p), ("record_iter", ctypes.c_void_p)]


PNP_REC = 232
_PNP_CORR_TAPS = (("p2d", np.float32, 2), ("p3d", np.float32, 3), ("max_err", np.float32, 0), ("kp_index", np.int32, 0))
_PNP_ITER_TAPS = (("sets", np.int32, 4), ("rec", np.float64, PNP_REC), ("count", np.int32, 0))
_PNP_REFIT_TAPS = (("refit_rec", np.float64, PNP_REC), ("refit_count", np.int32, 0), ("record_iter", np.int32, 0))


def pnp_query(frame, draws, n_iter=5, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4,
              th2=5.991, state=None, taps=False, cap=None):
    """A PnpQuery over numpy arrays and the arrays it points to (keep both
    alive while the query is used): (query, keep).  frame: a dict of keys
    (KEYPOINT), pos (n x 3), valid (n), cam (fx, fy, cx, cy) and sigma2 (the
    level table); None: the query of a device-resident candidate (cap
    keypoints; only the parameters, the state and the draws are read).
    draws: k x 4 rand() values.  state: the dict pnp_result returned for the
    solver's previous call (iter_done, best_inliers, best_mask, best_Tcw), or
    None for a fresh solver."""
    keep = {}
    q = PnpQuery()
    if frame is not None:
        keep["keys"] = np.ascontiguousarray(frame["keys"], KEYPOINT)
        keep["pos"] = np.ascontiguousarray(frame["pos"], np.float32).reshape(-1, 3)
        keep["valid"] = np.ascontiguousarray(frame["valid"], np.uint8)
        keep["cam"] = np.ascontiguousarray(frame["cam"], np.float32).reshape(-1)
        keep["sigma2"] = np.ascontiguousarray(frame["sigma2"], np.float32).reshape(-1)
        for name in ("keys", "pos", "valid", "cam", "sigma2"):
            setattr(q, name, keep[name].ctypes.data)
        q.n, q.nlevels = len(keep["keys"]), len(keep["sigma2"])
        if cap is None:
            cap = q.n
    q.cap = max(int(cap), 0)
    keep["draws"] = np.ascontiguousarray(draws, np.int32).reshape(-1, 4)
    q.draws, q.n_draws, q.n_iter = keep["draws"].ctypes.data, len(keep["draws"]), int(n_iter)
    q.probability, q.min_inliers, q.max_iterations, q.min_set = probability, min_inliers, max_iterations, min_set
    q.epsilon, q.th2 = epsilon, th2
    keep["inliers"] = np.zeros(max(q.cap, 1), np.uint8)
    keep["best_mask"] = np.zeros(max(q.cap, 1), np.uint8)
    if state is not None:
        q.iter_done, q.best_inliers = int(state["iter_done"]), int(state["best_inliers"])
        m = np.asarray(state["best_mask"], np.uint8)
        keep["best_mask"][:len(m)] = m
        q.best_Tcw = (ctypes.c_float * 16)(*np.asarray(state["best_Tcw"], np.float32).reshape(-1))
    q.inliers, q.best_mask = keep["inliers"].ctypes.data, keep["best_mask"].ctypes.data
    if taps:
        m = max(q.n_draws, 1)
        for name, dt, k in _PNP_CORR_TAPS:
            keep[name] = np.zeros((max(q.cap, 1), k) if k else max(q.cap, 1), dt)
        for name, dt, k in _PNP_ITER_TAPS:
            keep[name] = np.zeros((m, k) if k else m, dt)
        for name, dt, k in _PNP_REFIT_TAPS:
            keep[name] = np.zeros((m + 1, k) if k else m + 1, dt)
        for name, _, _ in _PNP_CORR_TAPS + _PNP_ITER_TAPS + _PNP_REFIT_TAPS:
            setattr(q, name, keep[name].ctypes.data)
    return q, keep


def pnp_result(q, keep, taps=False, n=None):
    """The out and state fields (and taps) of a filled PnpQuery as a dict."""
    n = q.n if n is None else n
    r = dict(N=q.N, ransac_min_inliers=q.ransac_min_inliers, ransac_max_its=q.ransac_max_its, iters_run=q.iters_run,
             no_more=q.no_more, found=q.found, found_iter=q.found_iter, n_inliers=q.n_inliers, refined=q.refined,
             n_records=q.n_records, best_slot=q.best_slot,
             Tcw=np.array(q.Tcw, np.float32) if q.found else None, inliers=keep["inliers"][:n].copy(),
             iter_done=q.iter_done, best_inliers=q.best_inliers, best_mask=keep["best_mask"][:n].copy(),
             best_Tcw=np.array(q.best_Tcw, np.float32))
    if taps:
        for name, _, _ in _PNP_CORR_TAPS:
            r[name] = keep[name][:q.N]
        for name, _, _ in _PNP_ITER_TAPS + _PNP_REFIT_TAPS:
            r[name] = keep[name]
    return r


class KfGeom(ctypes.Structure):
    """orbx_kf_geom (include/orbx.h)."""
    _fields_ = [("Rcw", ctypes.c_void_p), ("tcw", ctypes.c_void_p), ("Ow", ctypes.c_void_p), ("cam", ctypes.c_void_p),
                ("scale_factors", ctypes.c_void_p), ("level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int)]


class BowView(ctypes.Structure):
    """orbx_bow_view (include/orbx.h)."""
    _fields_ = [("keys", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("n", ctypes.c_int), ("mp", ctypes.c_void_p),
                ("n_nodes", ctypes.c_int), ("node_id", ctypes.c_void_p), ("node_ptr", ctypes.c_void_p),
                ("feat_idx", ctypes.c_void_p)]


def kf_geom(g):
    """A KfGeom over a dict of Rcw (3x3), tcw, Ow, cam (fx, fy, cx, cy),
    scale_factors and level_sigma2, and the float32 arrays it points to (keep
    them alive while the struct is used): (struct, keep)."""
    keep = {k: np.ascontiguousarray(g[k], np.float32).reshape(-1)
            for k in ("Rcw", "tcw", "Ow", "cam", "scale_factors", "level_sigma2")}
    q = KfGeom()
    for k, a in keep.items():
        setattr(q, k, a.ctypes.data)
    q.nlevels = int(g.get("nlevels", len(keep["scale_factors"])))
    return q, keep


def _geoms(gs):
    built = [kf_geom(g) for g in gs]
    return (KfGeom * max(len(built), 1))(*[b[0] for b in built]), built


def _ptr_array(arrays):
    return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def _new_points_outputs(n, length, v4):
    out = dict(xyz=[np.zeros((length, 3), np.float32) for _ in range(n)],
               status=[np.zeros(length, np.uint8) for _ in range(n)], n_created=np.zeros(max(n, 1), np.int32),
               v4=[np.zeros((length, 4), np.float32) for _ in range(n)] if v4 else None)
    return out


_lib = None


def lib():
    """Load liborbx.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise OrbxError(-2, f"liborbx.so missing at {LIB_PATH}; run python -m orb_slam_amd.build")
        _lib = ctypes.CDLL(str(LIB_PATH))
        _declare(_lib)
    return _lib


def _declare(L):
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    ip = ctypes.POINTER(ctypes.c_int)
    dp = ctypes.POINTER(ctypes.c_double)
    sigs = {
        "orbx_create": ([ctypes.POINTER(vp), i, i, f, i, i, i, i, i, i], i),
        "orbx_destroy": ([vp], None),
        "orbx_get_levels": ([vp], i),
        "orbx_get_scale_factor": ([vp], f),
        "orbx_get_features_per_level": ([vp, vp, i], i),
        "orbx_get_scale_factors": ([vp, vp, i], i),
        "orbx_extract": ([vp, vp, i, i, sz, vp, vp, i, ip], i),
        "orbx_extract_batch": ([vp, i, vp, i, i, sz, vp, vp, i, vp], i),
        "orbx_dev_upload": ([vp, i, i, vp, i, i, sz], i),
        "orbx_dev_extract": ([vp, i, i], i),
        "orbx_dev_match_prev": ([vp, i, i, i, i, f, i], i),
        "orbx_dev_sync": ([vp], i),
        "orbx_dev_match_bf_prev": ([vp, i, i, i, i, f], i),
        "orbx_dev_set_split": ([vp, i], i),
        "orbx_dev_set_async_match": ([vp, i], i),
        "orbx_set_fp_contract": ([vp, i], i),
        "orbx_get_fp_contract": ([vp], i),
        "orbx_set_nth_pivot": ([vp, i], i),
        "orbx_get_nth_pivot": ([vp], i),
        "orbx_dev_extract_match": ([vp, i, i, i, i, i, i, f, i], i),
        "orbx_dev_read_features": ([vp, i, vp, vp, i, ip], i),
        "orbx_dev_read_matches": ([vp, i, vp, i, ip, ip], i),
        "orbx_dev_kernel_time": ([vp, ctypes.c_char_p, dp, dp], i),
        "orbx_dev_kernel_time_enable": ([vp, i], i),
        "orbx_dev_kernel_time_select": ([vp, ctypes.c_char_p], i),
        "orbx_dev_read_level": ([vp, i, i, i, vp, i, ip, ip], i),
        "orbx_descriptor_distance": ([vp, vp], i),
        "orbx_hamming_bf": ([vp, vp, i, vp, i, vp, vp, vp], i),
        "orbx_match_bf": ([vp, vp, i, vp, i, i, f, vp, ip], i),
        "orbx_search_for_initialization": ([vp, vp, vp, vp, vp, i, f, i, ip], i),
        "orbx_window_search": ([vp, vp, vp, vp, i, i, i, f, i, vp, ip], i),
        "orbx_search_by_projection_pair": ([vp, vp, vp, vp, vp, vp, vp, vp, i, f, vp, ip], i),
        "orbx_search_by_projection_motion": ([vp, vp, vp, vp, vp, vp, vp, vp, f, i, vp, ip], i),
        "orbx_search_by_projection_local": ([vp, vp, i, vp, vp, vp, vp, vp, vp, f, f, vp, ip], i),
        "orbx_search_local_map": ([vp, vp], i),
        "orbx_search_local_map_batch": ([vp, i, vp], i),
        "orbx_track_frame": ([vp, vp], i),
        "orbx_lba_solve": ([vp, vp, i, i, vp, vp, vp, vp], i),
        "orbx_lba_solve_batch": ([vp, i, vp, i, i, vp, vp, vp, vp], i),
        "orbx_lba_stage": ([vp, i, vp], i),
        "orbx_lba_run": ([vp, i, i, vp], i),
        "orbx_lba_fetch": ([vp, vp, vp, vp, vp], i),
        "orbx_search_by_bow_frame": ([vp, vp, vp, f, i, vp, ip], i),
        "orbx_search_by_bow_kf": ([vp, vp, vp, f, i, vp, ip], i),
        "orbx_search_for_triangulation": ([vp, vp, vp, vp, vp, i, i, vp, ip], i),
        "orbx_search_for_triangulation_batch": ([vp, vp, i, vp, vp, vp, i, i, vp, vp], i),
        "orbx_search_by_bow_kf_batch": ([vp, vp, i, vp, f, i, vp, vp], i),
        "orbx_fuse_candidates_batch": ([vp, i, vp, vp, vp, vp, i, f, vp, vp], i),
        "orbx_fuse_candidates": ([vp, vp, vp, vp, vp, i, f, vp, vp], i),
        "orbx_dev_fuse_candidates": ([vp, i, vp, vp, vp, vp, vp, i, f, vp, vp], i),
        "orbx_dev_search_by_projection_kf_sim3": ([vp, i, vp, vp, vp, vp, vp, i, vp, i, ip], i),
        "orbx_dev_search_by_projection_frame_kf": ([vp, i, vp, i, vp, vp, vp, vp, vp, f, i, i, vp, i, ip], i),
        "orbx_dev_search_by_sim3": ([vp, i, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, f, vp, vp, f, vp, vp, i, ip], i),
        "orbx_search_by_sim3": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f, vp, vp, f, vp, vp, ip], i),
        "orbx_distinctive_descriptors": ([vp, i, vp, vp, vp], i),
        "orbx_search_by_projection_kf_sim3": ([vp, vp, vp, vp, vp, vp, i, vp, ip], i),
        "orbx_search_by_projection_frame_kf": ([vp, vp, vp, vp, vp, vp, vp, vp, f, i, i, vp, ip], i),
        "orbx_vocab_create": ([vp, i, i, i, vp, vp, vp, vp, ctypes.POINTER(vp)], i),
        "orbx_vocab_destroy": ([vp], None),
        "orbx_vocab_n_words": ([vp], i),
        "orbx_vocab_transform": ([vp, vp, i, vp, i, vp, vp, vp, vp, vp, ip, vp, vp, vp, ip], i),
        "orbx_dev_compute_bow": ([vp, vp, i, i, i], i),
        "orbx_dev_read_bow": ([vp, i, i, vp, vp, vp, vp, vp, ip, vp, vp, vp, ip], i),
        "orbx_dev_search_by_bow": ([vp, i, i, vp, f, i, vp, i, vp], i),
        "orbx_dev_search_by_bow_kf": ([vp, i, vp, i, vp, vp, f, i, vp, i, vp], i),
        "orbx_dev_search_for_triangulation": ([vp, i, vp, i, vp, vp, vp, vp, i, i, vp, i, vp], i),
        "orbx_undistort_keypoints": ([vp, i, vp, vp, vp, vp], i),
        "orbx_compute_image_bounds": ([i, i, vp, vp, vp], i),
        "orbx_dev_undistort": ([vp, i, i, vp, vp], i),
        "orbx_pose_optimization": ([vp, vp, ip, vp], i),
        "orbx_pose_optimization_batch": ([vp, i, vp, vp, vp], i),
        "orbx_pose_stage": ([vp, i, vp], i),
        "orbx_pose_run": ([vp], i),
        "orbx_pose_fetch": ([vp, vp, vp, vp], i),
        "orbx_version": ([], ctypes.c_char_p),
        "orbx_abi_version": ([], i),
        "orbx_lba_set_workgroups": ([vp, i], i),
        "orbx_lba_get_workgroups": ([vp], i),
        "orbx_lba_last_workgroups": ([vp], i),
        "orbx_debug_lba_split": ([vp, i, i, i, i], i),
        "orbx_debug_describe_patch": ([vp, i, i, i, i, vp], i),
        "orbx_debug_describe_moments": ([vp, i, i, i, i, vp], i),
        "orbx_debug_level0_direct": ([vp], i),
        "orbx_debug_fill_pyramid": ([vp, i, i, i], i),
        "orbx_debug_write_features": ([vp, i, vp, vp, i], i),
        "orbx_debug_fast_instance": ([vp, vp], i),
        "orbx_debug_fast_lists": ([vp, i, vp, i, vp, i, vp], i),
        "orbx_debug_fast_list_cap": ([vp, i], i),
        "orbx_debug_fast_paths": ([vp, i, vp, i, vp], i),
        "orbx_pose_set_exact": ([vp, i], i),
        "orbx_pose_get_exact": ([vp], i),
        "orbx_dev_set_image_bounds": ([vp, vp], i),
        "orbx_set_launch_mode": ([vp, i], i),
        "orbx_get_launch_mode": ([vp], i),
        "orbx_host_alloc": ([sz, ctypes.POINTER(vp)], i),
        "orbx_host_free": ([vp], None),
        "orbx_dev_upload_async": ([vp, i, i, vp, i, i, sz], i),
        "orbx_dev_download_async": ([vp, i, i, vp, vp, vp, vp, vp], i),
        "orbx_describe_levels": ([i, f, i, i, i, i, vp, i], i),
        "orbx_init_models": ([vp, vp], i),
        "orbx_init_models_batch": ([vp, i, vp], i),
        "orbx_dev_init_models": ([vp, i, i, i, f, i, vp], i),
        "orbx_dev_read_init_models": ([vp, i, vp], i),
        "orbx_init_reconstruct": ([vp, vp], i),
        "orbx_init_reconstruct_batch": ([vp, i, vp], i),
        "orbx_dev_init_reconstruct": ([vp, i, i, i, vp, f, f, i], i),
        "orbx_dev_read_init_reconstruct": ([vp, i, vp, ip], i),
        "orbx_triangulate_matches": ([vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp, vp, vp], i),
        "orbx_create_new_map_points": ([vp, vp, vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp], i),
        "orbx_dev_create_new_map_points": ([vp, i, vp, vp, i, vp, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, i], i),
        "orbx_sim3_ransac": ([vp, vp], i),
        "orbx_sim3_ransac_batch": ([vp, i, vp], i),
        "orbx_pnp_ransac": ([vp, vp], i),
        "orbx_pnp_ransac_batch": ([vp, i, vp], i),
        "orbx_dev_pnp_candidates": ([vp, i, i, vp, vp, vp, vp, i, f, i, i, vp, i, vp, vp, vp], i),
        "orbx_dev_sim3_candidates": ([vp, i, vp, i, vp, vp, f, i, i, ctypes.c_double, i, i, i, vp, vp, i, vp, vp, vp], i),
        "orbx_optimize_sim3": ([vp, vp], i),
        "orbx_optimize_sim3_batch": ([vp, i, vp], i),
        "orbx_dev_optimize_sim3": ([vp, i, vp, vp, i, vp, vp, vp], i),
        "orbx_optimize_essential_graph": ([vp, vp], i),
        "orbx_essgraph_plan": ([i, vp, i, i, vp, vp, vp, vp, vp, vp, vp], i),
        "orbx_kfdb_create": ([vp, i, i, ctypes.POINTER(vp)], i),
        "orbx_kfdb_destroy": ([vp], None),
        "orbx_kfdb_clear": ([vp, vp], i),
        "orbx_kfdb_size": ([vp], i),
        "orbx_kfdb_add": ([vp, vp, i, i, vp, vp], i),
        "orbx_kfdb_add_slot": ([vp, vp, i, i], i),
        "orbx_kfdb_erase": ([vp, vp, i], i),
        "orbx_kfdb_set_neighbours": ([vp, vp, i, vp, vp], i),
        "orbx_kfdb_query": ([vp, vp, vp], i),
        "orbx_kfdb_score": ([vp, vp, i, i, vp, vp, i, vp, vp], i),
        "orbx_covis_create": ([vp, i, i, i, ctypes.POINTER(vp)], i),
        "orbx_covis_destroy": ([vp], None),
        "orbx_covis_clear": ([vp, vp], i),
        "orbx_covis_size": ([vp], i),
        "orbx_covis_add_keyframe": ([vp, vp, i, ctypes.c_uint64, i, vp], i),
        "orbx_covis_set_matches": ([vp, vp, i, i, vp, vp], i),
        "orbx_covis_erase_points": ([vp, vp, i, vp], i),
        "orbx_covis_erase_keyframe": ([vp, vp, i], i),
        "orbx_covis_update_connections": ([vp, vp, i, vp, i, vp, vp], i),
        "orbx_covis_connections": ([vp, vp, i, i, vp, vp, i, ctypes.POINTER(i)], i),
        "orbx_covis_update_reference": ([vp, vp, vp], i),
        "orbx_covis_set_octaves": ([vp, vp, i, i, vp], i),
        "orbx_covis_cull_keyframes": ([vp, vp, vp], i),
        "orbx_covis_cull_points": ([vp, vp, i, i, vp, vp, vp, vp, vp], i),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _async_array(a, dtype, min_items, name):
    """An asynchronous copy's host array: a HostArray or numpy array of
    `dtype`, C-contiguous (the copy goes through its raw pointer), holding at
    least min_items elements (None: no size requirement); None passes."""
    if a is None:
        return None
    if isinstance(a, HostArray):
        a = a.array
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{name}: expected a numpy array or HostArray, got {type(a).__name__}")
    if a.dtype != np.dtype(dtype):
        raise TypeError(f"{name}: dtype {a.dtype}, expected {np.dtype(dtype)}")
    if not a.flags.c_contiguous:
        raise ValueError(f"{name}: must be C-contiguous")
    if min_items is not None and a.size < min_items:
        raise ValueError(f"{name}: {a.size} elements, the copy writes {min_items}")
    return a


def _check(code, where):
    if code != ORBX_OK:
        raise OrbxError(code, where)


class Context:
    """An orbx_ctx: one device, one HIP stream, `slots` device frame slots.

    Mirrors ORB_SLAM::ORBextractor(nfeatures, scaleFactor, nlevels,
    scoreType, fastTh) (include/ORBextractor.h:37) plus the batched,
    device-resident pipeline.
    """

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, score_type=1, fast_th=20,
                 max_w=640, max_h=480, slots=1, device=0):
        self._h = ctypes.c_void_p()
        self.nfeatures = nfeatures
        self.slots = slots
        _check(lib().orbx_create(ctypes.byref(self._h), device, nfeatures, scale_factor, nlevels,
                                 score_type, fast_th, max_w, max_h, slots), "orbx_create")

    def close(self):
        if self._h:
            lib().orbx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- ORBextractor API -------------------------------------------------
    def GetLevels(self):
        return lib().orbx_get_levels(self._h)

    def GetScaleFactor(self):
        return lib().orbx_get_scale_factor(self._h)

    def features_per_level(self):
        out = np.zeros(64, np.int32)
        n = lib().orbx_get_features_per_level(self._h, _ptr(out), 64)
        return out[:n]

    def __call__(self, image, mask=None):
        """ORBextractor::operator()(image, mask, keypoints, descriptors).

        `mask` is accepted and has no effect, as in the reference: it only
        feeds mvMaskPyramid (src/ORBextractor.cc:792-812), whose per-cell
        ROI (:601-603) FAST never reads (:607, :613)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape if img.ndim == 2 else (0, 0)
        kps = np.zeros(self.nfeatures, KEYPOINT)
        desc = np.zeros((self.nfeatures, 32), np.uint8)
        n = ctypes.c_int(0)
        _check(lib().orbx_extract(self._h, _ptr(img) if img.size else None, w, h, w, _ptr(kps),
                                  _ptr(desc), self.nfeatures, ctypes.byref(n)), "orbx_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def set_image_bounds(self, bounds=None):
        """orbx_dev_set_image_bounds: (min_x, max_x, min_y, max_y) of the
        slots' undistorted keypoints for the device matchers, None = image."""
        b = None if bounds is None else np.ascontiguousarray(bounds, np.float32)
        _check(lib().orbx_dev_set_image_bounds(self._h, _ptr(b)), "orbx_dev_set_image_bounds")

    def set_launch_mode(self, mode):
        """orbx_extract's launches: 1 one captured hipGraph per call (default),
        0 stream launches (orbx_set_launch_mode)."""
        _check(lib().orbx_set_launch_mode(self._h, int(mode)), "orbx_set_launch_mode")

    def launch_mode(self):
        return lib().orbx_get_launch_mode(self._h)

    # --- device-resident pipeline ------------------------------------------
    def upload(self, frames, first=0):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim == 2:
            frames = frames[None]
        cnt, h, w = frames.shape
        _check(lib().orbx_dev_upload(self._h, first, cnt, _ptr(frames), w, h, w), "orbx_dev_upload")

    def upload_async(self, frames, first=0):
        """orbx_dev_upload_async: `frames` (count, h, w) u8, C-contiguous --
        a HostArray (or its .array) for the copy to overlap device work.  The
        memory must stay untouched until the extraction of those slots."""
        frames = _async_array(frames, np.uint8, None, "frames")
        if frames.ndim != 3:
            raise ValueError(f"frames: expected (count, h, w), got shape {frames.shape}")
        cnt, h, w = frames.shape
        _check(lib().orbx_dev_upload_async(self._h, first, cnt, _ptr(frames), w, h, w), "orbx_dev_upload_async")

    def download_async(self, first, count, kps=None, desc=None, n_kps=None, m12=None, n_m=None):
        """orbx_dev_download_async into (preferably page-locked: HostArray)
        arrays: kps count*nfeatures KEYPOINT, desc count*nfeatures*32 u8,
        n_kps count i32, m12 count*nfeatures i32, n_m count i32 (each may be
        None).  The arrays are written when the copy completes (after the
        next call that orders after it, e.g. sync)."""
        nf = self.nfeatures
        kps = _async_array(kps, KEYPOINT, count * nf, "kps")
        desc = _async_array(desc, np.uint8, count * nf * 32, "desc")
        n_kps = _async_array(n_kps, np.int32, count, "n_kps")
        m12 = _async_array(m12, np.int32, count * nf, "m12")
        n_m = _async_array(n_m, np.int32, count, "n_m")
        _check(lib().orbx_dev_download_async(self._h, first, count, _ptr(kps), _ptr(desc), _ptr(n_kps), _ptr(m12),
                                             _ptr(n_m)), "orbx_dev_download_async")

    def extract(self, first, count):
        _check(lib().orbx_dev_extract(self._h, first, count), "orbx_dev_extract")

    def match_prev(self, first, count, seq_len, window=100, nnratio=0.9, check_ori=True):
        _check(lib().orbx_dev_match_prev(self._h, first, count, seq_len, window, nnratio,
                                         int(check_ori)), "orbx_dev_match_prev")

    def extract_match(self, first, count, seq_len, mode="init", window=100, th_low=50, nnratio=0.9,
                      check_ori=True):
        """Extract a batch and match each frame against its predecessor
        (mode "init": SearchForInitialization, "bf": brute force), pipelined."""
        _check(lib().orbx_dev_extract_match(self._h, first, count, seq_len, 1 if mode == "init" else 2, window,
                                            th_low, nnratio, int(check_ori)), "orbx_dev_extract_match")

    def set_split(self, enable):
        """Extraction pipeline parts for a batch (orbx_dev_set_split): 0 one
        stream, 1 the default three parts, 2-4 that many parts on their own
        streams."""
        _check(lib().orbx_dev_set_split(self._h, int(enable)), "orbx_dev_set_split")

    def set_fp_contract(self, enable):
        """Evaluate src/ORBextractor.cc's own float expressions (descriptor
        sample coordinates, Harris response) as a reference build with GCC's
        FMA contraction does (orbx_set_fp_contract)."""
        _check(lib().orbx_set_fp_contract(self._h, int(enable)), "orbx_set_fp_contract")

    def set_nth_pivot(self, mode):
        """retainBest's std::nth_element pivot step as libstdc++ >= 4.9 (0) or
        GCC 4.6 .. 4.8 (1, default: the reference's documented platforms)
        implements it (orbx_set_nth_pivot)."""
        _check(lib().orbx_set_nth_pivot(self._h, int(mode)), "orbx_set_nth_pivot")

    def nth_pivot(self):
        """The retainBest era in effect (orbx_get_nth_pivot)."""
        return lib().orbx_get_nth_pivot(self._h)

    def set_async_match(self, enable):
        """Queue extract_match's matching behind the extraction on an internal
        stream; later extract_match calls on other slots overlap it."""
        _check(lib().orbx_dev_set_async_match(self._h, int(enable)), "orbx_dev_set_async_match")

    def match_bf_prev(self, first, count, seq_len, th_low=50, nnratio=0.9):
        _check(lib().orbx_dev_match_bf_prev(self._h, first, count, seq_len, th_low, nnratio),
               "orbx_dev_match_bf_prev")

    def sync(self):
        _check(lib().orbx_dev_sync(self._h), "orbx_dev_sync")

    def features(self, slot):
        kps = np.zeros(self.nfeatures, KEYPOINT)
        desc = np.zeros((self.nfeatures, 32), np.uint8)
        n = ctypes.c_int(0)
        _check(lib().orbx_dev_read_features(self._h, slot, _ptr(kps), _ptr(desc), self.nfeatures,
                                            ctypes.byref(n)), "orbx_dev_read_features")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def write_features(self, slot, kps, desc):
        """Debug (orbx_debug_write_features): host keypoint records and
        descriptors become the slot's device outputs and count, so the slot
        matchers can be given inputs that extraction never produces."""
        kps = np.ascontiguousarray(kps, KEYPOINT)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(len(kps), 32)
        _check(lib().orbx_debug_write_features(self._h, slot, _ptr(kps) if len(kps) else None,
                                               _ptr(desc) if len(kps) else None, len(kps)),
               "orbx_debug_write_features")

    def matches(self, slot):
        m = np.zeros(self.nfeatures, np.int32)
        nm, n1 = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().orbx_dev_read_matches(self._h, slot, _ptr(m), self.nfeatures, ctypes.byref(nm),
                                           ctypes.byref(n1)), "orbx_dev_read_matches")
        return m, nm.value

    def level(self, slot, level, blurred=False, cap=4 << 20):
        buf = np.zeros(cap, np.uint8)
        pw, ph = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().orbx_dev_read_level(self._h, slot, level, int(blurred), _ptr(buf), cap,
                                         ctypes.byref(pw), ctypes.byref(ph)), "orbx_dev_read_level")
        return buf[:pw.value * ph.value].reshape(ph.value, pw.value).copy()

    def describe_patch(self, slot, level, x, y):
        """The blurred 37x37 patch that the describe kernel builds around
        level position (x, y) of the slot's pyramid (orbx_debug_describe_patch)."""
        out = np.zeros((37, 37), np.uint8)
        _check(lib().orbx_debug_describe_patch(self._h, slot, level, x, y, _ptr(out)), "orbx_debug_describe_patch")
        return out

    def describe_moments(self, slot, level, x, y):
        """IC_Angle's moments as the describe kernel computes them at level
        position (x, y) of the slot's pyramid: (m01, m10) of the wave's lower
        half and of its upper half (orbx_debug_describe_moments)."""
        out = np.zeros(4, np.int32)
        _check(lib().orbx_debug_describe_moments(self._h, slot, level, x, y, _ptr(out)), "orbx_debug_describe_moments")
        return (int(out[0]), int(out[1])), (int(out[2]), int(out[3]))

    def level0_direct(self):
        """Whether the last extraction read pyramid level 0 from the frame
        store, without the padded copy (orbx_debug_level0_direct)."""
        r = lib().orbx_debug_level0_direct(self._h)
        if r < 0:
            raise OrbxError(r, "orbx_debug_level0_direct")
        return bool(r)

    def fill_pyramid(self, first_slot, count, byte):
        """Debug (orbx_debug_fill_pyramid): fills the whole raw-pyramid area of
        slots [first_slot, first_slot + count) with one byte value, after all
        pending work.  Tests poison the areas with it: the batch extraction
        writes level interiors only and must not depend on any other byte."""
        _check(lib().orbx_debug_fill_pyramid(self._h, int(first_slot), int(count), int(byte)),
               "orbx_debug_fill_pyramid")

    def fast_instance(self):
        """The FAST kernel instance of the last extraction: (tile pitch, 0 for
        the runtime-pitch instance; workgroup threads; band rows, 0 for whole
        cells) (orbx_debug_fast_instance)."""
        out = np.zeros(3, np.int32)
        _check(lib().orbx_debug_fast_instance(self._h, _ptr(out)), "orbx_debug_fast_instance")
        return tuple(int(v) for v in out)

    def set_fast_list_cap(self, n):
        """Capacity of the FAST kernel's scored-pixel list for the context's
        later extractions (orbx_debug_fast_list_cap): n < 0 the default, 0
        every cell on the dword path."""
        _check(lib().orbx_debug_fast_list_cap(self._h, int(n)), "orbx_debug_fast_list_cap")

    def fast_paths(self, slot, cells_cap=1 << 14):
        """(paths, capacity) of a slot's last extraction
        (orbx_debug_fast_paths): per cell the paths its bands took (bit 0: the
        scored-pixel list, bit 1: the dword path) and the list capacity the
        launch ran with."""
        out = np.zeros(cells_cap, np.uint8)
        cap = ctypes.c_int(0)
        n = lib().orbx_debug_fast_paths(self._h, slot, _ptr(out), out.size, ctypes.byref(cap))
        _check(min(n, 0), "orbx_debug_fast_paths")
        return out[:n].copy(), cap.value

    def fast_lists(self, slot, cells_cap=1 << 14, lists_cap=1 << 22):
        """FAST's output for a slot before retainBest (orbx_debug_fast_lists):
        a list of (level, ini_x, ini_y, hx, hy, valid, corners) per cell,
        corners an (n, 3) int array of (level x, level y, score) in raster
        order."""
        cells = np.zeros(10 * cells_cap, np.int32)
        lists = np.zeros(lists_cap, np.uint32)
        ne = ctypes.c_int(0)
        n = lib().orbx_debug_fast_lists(self._h, slot, _ptr(cells), cells.size, _ptr(lists), lists.size,
                                        ctypes.byref(ne))
        _check(min(n, 0), "orbx_debug_fast_lists")
        out = []
        for level, ini_x, ini_y, hx, hy, valid, off, cap, cnt, _ in cells[:10 * n].reshape(n, 10):
            assert 0 <= cnt <= cap and off + cnt <= ne.value, (cnt, cap, off, ne.value)
            e = lists[off:off + cnt]
            xy = np.stack([e & 0xFFF, (e >> 12) & 0xFFF, e >> 24], axis=1).astype(np.int64)
            out.append((int(level), int(ini_x), int(ini_y), int(hx), int(hy), bool(valid), xy))
        return out

    def timing(self, enable=True, only=None):
        """Kernel timing with hipEvents around every launch, or only around
        the launches of timer `only`."""
        _check(lib().orbx_dev_kernel_time_select(self._h, only.encode() if only else None), "timing")
        _check(lib().orbx_dev_kernel_time_enable(self._h, int(enable)), "timing")

    def kernel_time(self, name):
        avg, tot = ctypes.c_double(0), ctypes.c_double(0)
        n = lib().orbx_dev_kernel_time(self._h, name.encode(), ctypes.byref(avg), ctypes.byref(tot))
        if n < 0:
            raise OrbxError(n, "orbx_dev_kernel_time")
        return n, avg.value, tot.value

    # --- Optimizer::PoseOptimization --------------------------------------
    def pose_optimization(self, frames):
        """Optimizer::PoseOptimization on a list of orbx_pose_frame structs
        (orb_slam_amd.synth_pose.to_ctypes): updates their Tcw / outlier in
        place, returns (n_inliers, stats)."""
        from .synth_pose import PoseStats
        arr = (type(frames[0]) * len(frames))(*frames)
        n = np.zeros(len(frames), np.int32)
        st = (PoseStats * len(frames))()
        _check(lib().orbx_pose_optimization_batch(self._h, len(frames), arr, _ptr(n), st),
               "orbx_pose_optimization_batch")
        for k in range(len(frames)):
            frames[k].Tcw = arr[k].Tcw
        return n, list(st)

    def pose_stage(self, frames):
        arr = (type(frames[0]) * len(frames))(*frames)
        _check(lib().orbx_pose_stage(self._h, len(frames), arr), "orbx_pose_stage")
        self._pose_staged = arr

    def pose_run(self):
        _check(lib().orbx_pose_run(self._h), "orbx_pose_run")

    def pose_fetch(self):
        from .synth_pose import PoseStats
        arr = self._pose_staged
        n = np.zeros(len(arr), np.int32)
        st = (PoseStats * len(arr))()
        _check(lib().orbx_pose_fetch(self._h, arr, _ptr(n), st), "orbx_pose_fetch")
        return arr, n, list(st)

    # --- DBoW2 on device-resident frames -----------------------------------
    def compute_bow(self, voc, first, count, levelsup=4):
        """Frame::ComputeBoW of extracted slots [first, first+count) on the
        device (orbx_dev_compute_bow); `voc` is a Vocabulary."""
        _check(lib().orbx_dev_compute_bow(self._h, voc.handle, first, count, levelsup), "orbx_dev_compute_bow")

    def read_bow(self, slot):
        """(BowVector, FeatureVector, per-feature (word, weight, node)) of a
        slot as numpy arrays: bow = (words, values); fv = (node ids, CSR
        offsets, feature indices)."""
        n = self.nfeatures
        word, weight, node = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32)
        bw, bv = np.zeros(n, np.uint32), np.zeros(n)
        fn, fp, ff = np.zeros(n, np.uint32), np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
        nw, nf = ctypes.c_int(), ctypes.c_int()
        _check(lib().orbx_dev_read_bow(self._h, slot, n, _ptr(word), _ptr(weight), _ptr(node), _ptr(bw), _ptr(bv),
                                       ctypes.byref(nw), _ptr(fn), _ptr(fp), _ptr(ff), ctypes.byref(nf)),
               "orbx_dev_read_bow")
        m = int(fp[nf.value])
        return ((bw[:nw.value].copy(), bv[:nw.value].copy()), (fn[:nf.value].copy(), fp[:nf.value + 1].copy(),
                                                               ff[:m].copy()), (word, weight, node))

    def search_by_bow(self, slot, kf_views, nnratio=0.75, check_ori=True):
        """Tracking::Relocalisation's SearchByBoW(pKF, F) loop against the
        frame in `slot` (orbx_dev_search_by_bow): kf_views are orbx_bow_view
        ctypes structures.  Returns (matches per keyframe, counts)."""
        n = len(kf_views)
        outs = [np.zeros(self.nfeatures, np.int32) for _ in range(n)]
        ptrs = (ctypes.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        arr = (type(kf_views[0]) * n)(*kf_views) if n else None
        nm = np.zeros(max(n, 1), np.int32)
        _check(lib().orbx_dev_search_by_bow(self._h, slot, n, arr, nnratio, int(check_ori), ptrs, self.nfeatures,
                                            _ptr(nm)), "orbx_dev_search_by_bow")
        return outs, nm[:n]

    # --- Initializer: homography / fundamental models ----------------------
    def init_models(self, keys1, keys2, matches12, draws, sigma=1.0, max_iter=200, taps=False):
        """Initializer::FindHomography + FindFundamental and the score ratio
        (orbx_init_models): a dict of n_matches, best_h / best_f, SH, SF, RH,
        H21 / F21 (None without a winner), inliers_h / inliers_f and, with
        taps, the per-iteration arrays of orbx_init_query."""
        q, keep = init_query(keys1, keys2, matches12, draws, sigma, max_iter, taps)
        _check(lib().orbx_init_models(self._h, ctypes.byref(q)), "orbx_init_models")
        return init_result(q, keep, taps)

    def init_models_batch(self, queries, taps=False):
        """orbx_init_models_batch over (keys1, keys2, matches12, draws, sigma,
        max_iter) tuples: one upload, one read-back; a list of dicts."""
        built = [init_query(*a, taps=taps) for a in queries]
        arr = (InitQuery * len(built))(*[b[0] for b in built])
        _check(lib().orbx_init_models_batch(self._h, len(built), arr), "orbx_init_models_batch")
        return [init_result(arr[k], built[k][1], taps) for k in range(len(built))]

    def dev_init_models(self, first, count, seq_len, draws, sigma=1.0, max_iter=200):
        """orbx_dev_init_models: the models of every pair (s - 1, s) of slots
        [first, first + count) from the slots' keypoints and matches; draws
        (count, max_iter, 8) int32."""
        d = np.ascontiguousarray(draws, np.int32)
        if d.size != count * max_iter * 8:
            raise ValueError(f"draws: {d.size} values, expected count x max_iter x 8 = {count * max_iter * 8}")
        _check(lib().orbx_dev_init_models(self._h, first, count, seq_len, sigma, max_iter, _ptr(d)),
               "orbx_dev_init_models")
        self._init_iter = max_iter

    def read_init_models(self, slot, taps=False):
        """orbx_dev_read_init_models: the dict of init_models for the pair
        (slot - 1, slot) of the last dev_init_models run."""
        q, keep = init_query(None, None, None, None, max_iter=getattr(self, "_init_iter", 1), taps=taps,
                             cap=self.nfeatures)
        _check(lib().orbx_dev_read_init_models(self._h, slot, ctypes.byref(q)), "orbx_dev_read_init_models")
        return init_result(q, keep, taps)

    # --- Initializer: ReconstructH / ReconstructF ---------------------------
    def init_reconstruct(self, keys1, keys2, matches12, inliers, model, M21, cam, sigma=1.0, min_parallax=1.0,
                         min_triangulated=50, taps=False):
        """Initializer::ReconstructH (model 0) / ReconstructF (model 1)
        (orbx_init_reconstruct): a dict of ok, n_inliers, n_hyp, best, R21 /
        t21 (None when not ok), n_good, parallax, p3d, triangulated and, with
        taps, svd, R_all, t_all, v4 and cos_parallax."""
        q, keep = reconstruct_query(keys1, keys2, matches12, inliers, model, M21, cam, sigma, min_parallax,
                                    min_triangulated, taps)
        _check(lib().orbx_init_reconstruct(self._h, ctypes.byref(q)), "orbx_init_reconstruct")
        return reconstruct_result(q, keep, taps)

    def init_reconstruct_batch(self, queries, taps=False):
        """orbx_init_reconstruct_batch over argument tuples of
        init_reconstruct: one upload, one read-back; a list of dicts."""
        built = [reconstruct_query(*a, taps=taps) for a in queries]
        arr = (ReconstructQuery * len(built))(*[b[0] for b in built])
        _check(lib().orbx_init_reconstruct_batch(self._h, len(built), arr), "orbx_init_reconstruct_batch")
        return [reconstruct_result(arr[k], built[k][1], taps) for k in range(len(built))]

    def dev_init_reconstruct(self, first, count, seq_len, cam, rh_threshold=None, min_parallax=1.0,
                             min_triangulated=50):
        """orbx_dev_init_reconstruct: the reconstruction of every pair of the
        last dev_init_models run on the same slots, from what that run left
        on the device.  rh_threshold None: RH_THRESHOLD, with which the
        device's float RH > rh_threshold is the reference's RH > 0.40."""
        if rh_threshold is None:
            rh_threshold = RH_THRESHOLD
        c = np.ascontiguousarray(cam, np.float32).reshape(-1)
        _check(lib().orbx_dev_init_reconstruct(self._h, first, count, seq_len, _ptr(c), rh_threshold, min_parallax,
                                               min_triangulated), "orbx_dev_init_reconstruct")

    def read_init_reconstruct(self, slot, taps=False, n_matches=None):
        """orbx_dev_read_init_reconstruct: the dict of init_reconstruct for
        the pair (slot - 1, slot) of the last dev_init_reconstruct run, with
        the chosen `model`.  The taps by match index are laid out by the
        pair's number of matches, which is read from the models run
        (read_init_models); a caller that passes n_matches must pass that
        number.  p3d / triangulated have one entry per feature of the context."""
        if taps:
            n = self.read_init_models(slot)["n_matches"]
            if n_matches is not None and n_matches != n:
                raise ValueError(f"read_init_reconstruct: n_matches {n_matches}, the pair has {n}")
            n_matches = n
        q, keep = reconstruct_query(None, None, None, None, 0, None, None, taps=taps, cap=self.nfeatures,
                                    n_max=self.nfeatures)
        model = ctypes.c_int(-1)
        _check(lib().orbx_dev_read_init_reconstruct(self._h, slot, ctypes.byref(q), ctypes.byref(model)),
               "orbx_dev_read_init_reconstruct")
        r = reconstruct_result(q, keep, taps, n1=self.nfeatures, n_matches=n_matches)
        r["model"] = model.value
        return r

    # --- LocalMapping::CreateNewMapPoints ----------------------------------
    def triangulate_matches(self, keys1, g1, keys2, g2s, matches12, v4=False):
        """orbx_triangulate_matches: the gates and the triangulation of
        src/LocalMapping.cc:283-368 for the matches of KF1 (keys1, geometry
        dict g1: kf_geom) against n neighbours (lists keys2, g2s, matches12).
        A dict of per-neighbour lists xyz (n1 x 3), status (n1) and, with
        v4, the null-vector tap (n1 x 4), and the array n_created."""
        n = len(keys2)
        k1 = np.ascontiguousarray(keys1, KEYPOINT)
        k2 = [np.ascontiguousarray(k, KEYPOINT) for k in keys2]
        m = [np.ascontiguousarray(a, np.int32) for a in matches12]
        if any(len(a) != len(k1) for a in m):
            raise ValueError("matches12: one entry per KF1 keypoint")
        G1, keep1 = kf_geom(g1)
        G2, keep2 = _geoms(g2s)
        n2 = np.array([len(k) for k in k2] + [0], np.int32)
        out = _new_points_outputs(n, len(k1), v4)
        _check(lib().orbx_triangulate_matches(self._h, _ptr(k1), len(k1), ctypes.byref(G1), n, _ptr_array(k2),
                                              _ptr(n2), G2, _ptr_array(m), _ptr_array(out["xyz"]),
                                              _ptr_array(out["status"]), _ptr(out["n_created"]),
                                              _ptr_array(out["v4"]) if v4 else None), "orbx_triangulate_matches")
        out["n_created"] = out["n_created"][:n]
        return out

    def create_new_map_points(self, KF1, g1, KF2s, g2s, F12s, check_ori=False, chain=True, v4=False):
        """orbx_create_new_map_points: SearchForTriangulation of the
        orbx_bow_view KF1 against the views KF2s and the triangulation of
        its matches; chain: the reference's loop, a created point marking its
        KF1 keypoint for the later neighbours.  The dict of
        triangulate_matches plus matches12 (list) and n_matches."""
        n = len(KF2s)
        G1, keep1 = kf_geom(g1)
        G2, keep2 = _geoms(g2s)
        F = np.ascontiguousarray(F12s, np.float32)
        if F.size != 9 * n:
            raise ValueError(f"F12s: {F.size} values, expected n x 9 = {9 * n}")
        arr = (type(KF1) * max(n, 1))(*KF2s)
        out = _new_points_outputs(n, KF1.n, v4)
        out["matches12"] = [np.full(KF1.n, -1, np.int32) for _ in range(n)]
        out["n_matches"] = np.zeros(max(n, 1), np.int32)
        _check(lib().orbx_create_new_map_points(self._h, ctypes.byref(KF1), ctypes.byref(G1), n, arr, G2, _ptr(F),
                                                int(check_ori), int(chain), _ptr_array(out["matches12"]),
                                                _ptr(out["n_matches"]), _ptr_array(out["xyz"]),
                                                _ptr_array(out["status"]), _ptr(out["n_created"]),
                                                _ptr_array(out["v4"]) if v4 else None),
               "orbx_create_new_map_points")
        out["n_created"], out["n_matches"] = out["n_created"][:n], out["n_matches"][:n]
        return out

    def dev_create_new_map_points(self, slot1, mp1, g1, slots2, mp2s, g2s, F12s, check_ori=False, chain=True,
                                  v4=False, cap=None):
        """orbx_dev_create_new_map_points: the same between device-resident
        frames (after extract and compute_bow on every slot named); mp1 /
        mp2s are the map-point states of the slots' keypoints.  Arrays of
        `cap` (default nfeatures) entries."""
        n = len(slots2)
        cap = self.nfeatures if cap is None else int(cap)
        G1, keep1 = kf_geom(g1)
        G2, keep2 = _geoms(g2s)
        F = np.ascontiguousarray(F12s, np.float32)
        if F.size != 9 * n:
            raise ValueError(f"F12s: {F.size} values, expected n x 9 = {9 * n}")
        m1 = np.ascontiguousarray(mp1, np.uint8)
        m2 = [np.ascontiguousarray(m, np.uint8) for m in mp2s]
        s2 = np.ascontiguousarray(list(slots2) + [0], np.int32)
        out = _new_points_outputs(n, max(cap, 1), v4)
        out["matches12"] = [np.full(max(cap, 1), -1, np.int32) for _ in range(n)]
        out["n_matches"] = np.zeros(max(n, 1), np.int32)
        _check(lib().orbx_dev_create_new_map_points(self._h, slot1, _ptr(m1), ctypes.byref(G1), n, _ptr(s2),
                                                    _ptr_array(m2), G2, _ptr(F), int(check_ori), int(chain),
                                                    _ptr_array(out["matches12"]), _ptr(out["n_matches"]),
                                                    _ptr_array(out["xyz"]), _ptr_array(out["status"]),
                                                    _ptr(out["n_created"]), _ptr_array(out["v4"]) if v4 else None,
                                                    cap), "orbx_dev_create_new_map_points")
        out["n_created"], out["n_matches"] = out["n_created"][:n], out["n_matches"][:n]
        return out

    # --- Tracking::Relocalisation: PnPsolver --------------------------------
    def pnp_ransac(self, frame, draws, taps=False, **kw):
        """One PnPsolver::iterate call on the device (orbx_pnp_ransac):
        arguments as pnp_query, a dict of the query's out and state fields
        (Tcw None when nothing was returned); pass it back as state= to
        continue the solver."""
        q, keep = pnp_query(frame, draws, taps=taps, **kw)
        _check(lib().orbx_pnp_ransac(self._h, ctypes.byref(q)), "orbx_pnp_ransac")
        return pnp_result(q, keep, taps)

    def pnp_ransac_batch(self, queries, taps=False):
        """orbx_pnp_ransac_batch over (frame, draws, kwargs) tuples: one
        upload, one launch set, one read-back."""
        built = [pnp_query(*a[:2], taps=taps, **(a[2] if len(a) > 2 else {})) for a in queries]
        arr = (PnpQuery * len(built))(*[b[0] for b in built])
        _check(lib().orbx_pnp_ransac_batch(self._h, len(built), arr), "orbx_pnp_ransac_batch")
        return [pnp_result(arr[k], built[k][1], taps) for k in range(len(built))]

    def dev_pnp_candidates(self, slot, kf_views, pos, cam, sigma2, draws, min_matches=15, nnratio=0.75,
                           check_ori=True, states=None, taps=False, **params):
        """orbx_dev_pnp_candidates: SearchByBoW(pKF, F) of the keyframe views
        (orbx_bow_view structures) against the frame in `slot` and a PnPsolver
        per candidate on the matches where the search left them.  pos: per
        candidate the keyframe's n x 3 GetWorldPos(); draws: per candidate
        k x 4 rand() values; states: per candidate None or the previous
        result; params as pnp_query.  Returns a dict: matches_f, n_matches,
        discarded, results (one dict per candidate, as pnp_ransac)."""
        n = len(kf_views)
        cap = self.nfeatures
        pos = [np.ascontiguousarray(p, np.float32).reshape(-1, 3) for p in pos]
        cam = np.ascontiguousarray(cam, np.float32).reshape(-1)
        sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        outs = [pnp_query(None, draws[k], state=states[k] if states else None, taps=taps, cap=cap, **params)
                for k in range(n)]
        arr = (PnpQuery * max(n, 1))(*[o[0] for o in outs])
        views = (type(kf_views[0]) * n)(*kf_views) if n else None
        m = [np.zeros(max(cap, 1), np.int32) for _ in range(n)]
        nm, disc = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        _check(lib().orbx_dev_pnp_candidates(self._h, slot, n, views, _ptr_array(pos), _ptr(cam), _ptr(sigma2),
                                             len(sigma2), nnratio, int(check_ori), int(min_matches), _ptr_array(m),
                                             cap, _ptr(nm), _ptr(disc), arr), "orbx_dev_pnp_candidates")
        return dict(matches_f=m, n_matches=nm[:n], discarded=disc[:n],
                    results=[pnp_result(arr[k], outs[k][1], taps, n=max(cap, 1)) for k in range(n)])

    # --- LoopClosing::ComputeSim3: Sim3Solver --------------------------------
    def sim3_ransac(self, kf1, kf2, matches12, draws, taps=False, **kw):
        """One Sim3Solver::iterate call on the device (orbx_sim3_ransac):
        arguments as sim3_query, a dict of the query's out fields (T12 None
        when nothing was returned, R12 / t12 / s12 None when no iteration of
        the call reached best_inliers) and, with taps, its tap arrays."""
        q, keep = sim3_query(kf1, kf2, matches12, draws, taps=taps, **kw)
        _check(lib().orbx_sim3_ransac(self._h, ctypes.byref(q)), "orbx_sim3_ransac")
        return sim3_result(q, keep, taps)

    def sim3_ransac_batch(self, queries, taps=False):
        """orbx_sim3_ransac_batch over (kf1, kf2, matches12, draws, kwargs)
        tuples: one upload, one launch set, one read-back; a list of dicts."""
        built = [sim3_query(*a[:4], taps=taps, **(a[4] if len(a) > 4 else {})) for a in queries]
        arr = (Sim3Query * len(built))(*[b[0] for b in built])
        _check(lib().orbx_sim3_ransac_batch(self._h, len(built), arr), "orbx_sim3_ransac_batch")
        return [sim3_result(arr[k], built[k][1], taps) for k in range(len(built))]

    def dev_sim3_candidates(self, slot1, kf1, slots2, kf2s, draws, n_iter=None, nnratio=0.75, check_ori=True,
                            min_matches=20, probability=0.99, min_inliers=20, max_iterations=300, states=None,
                            taps=False, cap=None):
        """orbx_dev_sim3_candidates: SearchByBoW of the keyframe in slot1
        against those in slots2 and a Sim3Solver per candidate on the matches
        the search left on the device.  kf1 / kf2s: dicts of mp (states 0, 1,
        2 per keypoint), pos, Tcw, cam, sigma2; draws (n, n_iter, 3); states:
        per candidate (iter_done, best_inliers), default (0, 0).  A dict of
        matches12 (list), n_matches, discarded and results (list of dicts as
        sim3_ransac)."""
        n = len(slots2)
        cap = self.nfeatures if cap is None else int(cap)
        d = np.ascontiguousarray(draws, np.int32)
        if n_iter is None:
            n_iter = d.size // (3 * max(n, 1))
        if d.size != n * n_iter * 3:
            raise ValueError(f"draws: {d.size} values, expected n x n_iter x 3 = {n * n_iter * 3}")

        def kf(g):
            keep = dict(mp=np.ascontiguousarray(g["mp"], np.uint8), pos=np.ascontiguousarray(g["pos"], np.float32),
                        Tcw=np.ascontiguousarray(g["Tcw"], np.float32).reshape(-1),
                        cam=np.ascontiguousarray(g["cam"], np.float32).reshape(-1),
                        sigma2=np.ascontiguousarray(g["sigma2"], np.float32).reshape(-1))
            k = Sim3Kf()
            for name, a in keep.items():
                setattr(k, name, a.ctypes.data)
            k.nlevels = int(g.get("nlevels", len(keep["sigma2"])))
            return k, keep
        K1, keep1 = kf(kf1)
        built2 = [kf(g) for g in kf2s]
        K2 = (Sim3Kf * max(n, 1))(*[b[0] for b in built2])
        outs = [sim3_query(None, None, None, None, n_iter=n_iter, taps=taps, cap=cap,
                           iter_done=states[k][0] if states else 0, best_inliers=states[k][1] if states else 0)
                for k in range(n)]
        arr = (Sim3Query * max(n, 1))(*[o[0] for o in outs])
        m12 = [np.full(max(cap, 1), -1, np.int32) for _ in range(n)]
        nm, disc = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        s2 = np.ascontiguousarray(list(slots2) + [0], np.int32)
        _check(lib().orbx_dev_sim3_candidates(self._h, slot1, ctypes.byref(K1), n, _ptr(s2), K2, nnratio,
                                              int(check_ori), min_matches, probability, min_inliers, max_iterations,
                                              n_iter, _ptr(d), _ptr_array(m12), cap, _ptr(nm), _ptr(disc), arr),
               "orbx_dev_sim3_candidates")
        return dict(matches12=m12, n_matches=nm[:n], discarded=disc[:n],
                    results=[sim3_result(arr[k], outs[k][1], taps, n1=max(cap, 1)) for k in range(n)])

    # --- LoopClosing::ComputeSim3: Optimizer::OptimizeSim3 --------------------
    def optimize_sim3(self, kf1, kf2, matches12, R12, t12, s12, th2=10.0, taps=False):
        """Optimizer::OptimizeSim3 on the device (orbx_optimize_sim3):
        arguments as sim3_opt_query, a dict as sim3_opt_result (matches12 is
        the cleared copy; the caller's array is left alone)."""
        q, keep = sim3_opt_query(kf1, kf2, matches12, R12, t12, s12, th2=th2, taps=taps)
        _check(lib().orbx_optimize_sim3(self._h, ctypes.byref(q)), "orbx_optimize_sim3")
        return sim3_opt_result(q, keep, taps)

    def optimize_essential_graph(self, kfs, edges, loop_kf, cur_kf, pos=None, ref_kf=None, taps=False):
        """Optimizer::OptimizeEssentialGraph on the device
        (orbx_optimize_essential_graph): arguments as essgraph_query, a dict as
        essgraph_result (Tcw n_kf x 12, pos, est n_kf x 8, the solver's counts
        and structure, the taps)."""
        q, keep = essgraph_query(kfs, edges, loop_kf, cur_kf, pos=pos, ref_kf=ref_kf, taps=taps)
        _check(lib().orbx_optimize_essential_graph(self._h, ctypes.byref(q)), "orbx_optimize_essential_graph")
        return essgraph_result(q, keep, taps)

    def optimize_sim3_batch(self, queries, th2=10.0, taps=False):
        """orbx_optimize_sim3_batch over (kf1, kf2, matches12, R12, t12, s12)
        tuples: one upload, one launch, one read-back; a list of dicts."""
        built = [sim3_opt_query(*a[:6], th2=th2, taps=taps) for a in queries]
        arr = (Sim3OptQuery * len(built))(*[b[0] for b in built])
        _check(lib().orbx_optimize_sim3_batch(self._h, len(built), arr), "orbx_optimize_sim3_batch")
        return [sim3_opt_result(arr[k], built[k][1], taps) for k in range(len(built))]

    def dev_optimize_sim3(self, slot1, kf1, slots2, kf2s, matches12, sims, th2=10.0, taps=False):
        """orbx_dev_optimize_sim3: OptimizeSim3 of the keyframe in slot1
        against those in slots2, keypoints and octaves read from the slots.
        kf1 / kf2s: dicts of mp (states 0, 1, 2 per keypoint), pos, Tcw, cam;
        kf1 also inv_sigma2, each of kf2s sigma2.  matches12: one array per
        candidate (an entry per keypoint of slot1); sims: (R12, t12, s12) per
        candidate.  A list of dicts as optimize_sim3."""
        n = len(slots2)

        def kf(g, table):
            keep = dict(mp=np.ascontiguousarray(g["mp"], np.uint8), pos=np.ascontiguousarray(g["pos"], np.float32),
                        Tcw=np.ascontiguousarray(g["Tcw"], np.float32).reshape(-1),
                        cam=np.ascontiguousarray(g["cam"], np.float32).reshape(-1),
                        sigma2=np.ascontiguousarray(g[table], np.float32).reshape(-1))
            k = Sim3Kf()
            for name, a in keep.items():
                setattr(k, name, a.ctypes.data)
            k.nlevels = int(g.get("nlevels", len(keep["sigma2"])))
            return k, keep
        K1, keep1 = kf(kf1, "inv_sigma2")
        built2 = [kf(g, "sigma2") for g in kf2s]
        K2 = (Sim3Kf * max(n, 1))(*[b[0] for b in built2])
        outs = [sim3_opt_query(None, None, matches12[k], *sims[k], th2=th2, taps=taps) for k in range(n)]
        arr = (Sim3OptQuery * max(n, 1))(*[o[0] for o in outs])
        s2 = np.ascontiguousarray(list(slots2) + [0], np.int32)
        _check(lib().orbx_dev_optimize_sim3(self._h, slot1, ctypes.byref(K1), _ptr(keep1["sigma2"]), n, _ptr(s2), K2,
                                            arr), "orbx_dev_optimize_sim3")
        return [sim3_opt_result(arr[k], outs[k][1], taps) for k in range(n)]

    @property
    def handle(self):
        return self._h


class HostArray:
    """Page-locked host memory from orbx_host_alloc viewed as a numpy array
    (freed with the object)."""

    def __init__(self, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        self._p = ctypes.c_void_p()
        _check(lib().orbx_host_alloc(max(n, 1), ctypes.byref(self._p)), "orbx_host_alloc")
        buf = (ctypes.c_uint8 * max(n, 1)).from_address(self._p.value)
        self.array = np.frombuffer(buf, np.uint8, count=n).view(dtype).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            lib().orbx_host_free(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Vocabulary:
    """A DBoW2 vocabulary tree in HBM (orbx_vocab_create): nodes as
    TemplatedVocabulary::loadFromTextFile lists them -- parent id per node
    (node 0 the root), leaf flags, 32-byte descriptors and weights."""

    def __init__(self, ctx, k, L, parent, is_leaf, desc, weight):
        self._keep = [np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(is_leaf, np.uint8),
                      np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(weight, np.float64)]
        self._h = ctypes.c_void_p()
        _check(lib().orbx_vocab_create(ctx.handle, k, L, len(self._keep[0]), *[_ptr(a) for a in self._keep],
                                       ctypes.byref(self._h)), "orbx_vocab_create")

    @property
    def handle(self):
        return self._h

    def n_words(self):
        return lib().orbx_vocab_n_words(self._h)

    def close(self):
        if self._h:
            lib().orbx_vocab_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KfdbQuery(ctypes.Structure):
    """orbx_kfdb_query_args (include/orbx.h)."""
    _fields_ = [("mode", ctypes.c_int), ("slot", ctypes.c_int), ("n_words", ctypes.c_int),
                ("words", ctypes.c_void_p), ("values", ctypes.c_void_p), ("min_score", ctypes.c_float),
                ("n_ref", ctypes.c_int), ("ref", ctypes.c_void_p), ("n_exclude", ctypes.c_int),
                ("exclude", ctypes.c_void_p), ("candidates", ctypes.c_void_p), ("cap", ctypes.c_int),
                ("n_candidates", ctypes.c_int), ("min_score_used", ctypes.c_float),
                ("max_common_words", ctypes.c_int), ("n_sharing", ctypes.c_int), ("n_scored", ctypes.c_int),
                ("tap_words", ctypes.c_void_p), ("tap_score", ctypes.c_void_p), ("tap_acc", ctypes.c_void_p),
                ("tap_best", ctypes.c_void_p), ("tap_pos", ctypes.c_void_p)]


KFDB_RELOC, KFDB_LOOP = 0, 1
KFDB_MAX_MEMBERS, KFDB_MAX_WORDS, KFDB_NEIGHBOURS = 8192, 4096, 10
_KFDB_TAPS = (("words", np.int32), ("score", np.float32), ("acc", np.float32), ("best", np.int32), ("pos", np.int32))


class KeyFrameDatabase:
    """ORB_SLAM::KeyFrameDatabase in HBM (orbx_kfdb_*): members are named by
    the caller's ids in [0, capacity) (KeyFrame::mnId).  A query is a slot of
    the context (an int: the BowVector compute_bow left there) or a
    (words, values) pair of arrays, words ascending."""

    def __init__(self, ctx, capacity, max_words):
        self._ctx = ctx
        self.capacity, self.max_words = int(capacity), int(max_words)
        self._h = ctypes.c_void_p()
        _check(lib().orbx_kfdb_create(ctx.handle, capacity, max_words, ctypes.byref(self._h)), "orbx_kfdb_create")

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().orbx_kfdb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return lib().orbx_kfdb_size(self._h)

    def clear(self):
        _check(lib().orbx_kfdb_clear(self._ctx.handle, self._h), "orbx_kfdb_clear")

    @staticmethod
    def _bow(bow):
        w = np.ascontiguousarray(bow[0], np.uint32).reshape(-1)
        v = np.ascontiguousarray(bow[1], np.float64).reshape(-1)
        if len(w) != len(v):
            raise ValueError("a BowVector has as many values as words")
        return w, v

    def add(self, kf_id, words, values):
        """KeyFrameDatabase::add from host arrays."""
        w, v = self._bow((words, values))
        _check(lib().orbx_kfdb_add(self._ctx.handle, self._h, int(kf_id), len(w), _ptr(w), _ptr(v)), "orbx_kfdb_add")

    def add_slot(self, kf_id, slot):
        """add of the BowVector compute_bow left in `slot` (device to device)."""
        _check(lib().orbx_kfdb_add_slot(self._ctx.handle, self._h, int(kf_id), int(slot)), "orbx_kfdb_add_slot")

    def erase(self, kf_id):
        _check(lib().orbx_kfdb_erase(self._ctx.handle, self._h, int(kf_id)), "orbx_kfdb_erase")

    def set_neighbours(self, ids, neigh):
        """GetBestCovisibilityKeyFrames(10) of members `ids`: a list of id
        lists (at most 10 each) or an n x 10 array padded with -1."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        rows = np.full((len(ids), KFDB_NEIGHBOURS), -1, np.int32)
        for k, row in enumerate(neigh):
            row = np.asarray(row, np.int32).reshape(-1)
            if len(row) > KFDB_NEIGHBOURS:
                raise ValueError("a neighbour row holds at most 10 ids")
            rows[k, :len(row)] = row
        _check(lib().orbx_kfdb_set_neighbours(self._ctx.handle, self._h, len(ids), _ptr(ids), _ptr(rows)),
               "orbx_kfdb_set_neighbours")

    def _query_bow(self, query):
        if isinstance(query, (int, np.integer)):
            return int(query), 0, None, None
        w, v = self._bow(query)
        return -1, len(w), w, v

    def score(self, query, ids):
        """mpVoc->score(query, member) as float32 for the named members."""
        slot, n, w, v = self._query_bow(query)
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        out = np.zeros(len(ids), np.float32)
        _check(lib().orbx_kfdb_score(self._ctx.handle, self._h, slot, n, _ptr(w) if n else None,
                                     _ptr(v) if n else None, len(ids), _ptr(ids), _ptr(out)), "orbx_kfdb_score")
        return out

    def _detect(self, mode, query, min_score, ref, exclude, taps, cap):
        q = KfdbQuery()
        q.mode = mode
        q.slot, q.n_words, w, v = self._query_bow(query)
        if q.n_words:
            q.words, q.values = w.ctypes.data, v.ctypes.data
        ref = np.ascontiguousarray(ref, np.int32).reshape(-1)
        exclude = np.ascontiguousarray(exclude, np.int32).reshape(-1)
        q.min_score, q.n_ref, q.n_exclude = float(min_score), len(ref), len(exclude)
        q.ref, q.exclude = (ref.ctypes.data if len(ref) else None), (exclude.ctypes.data if len(exclude) else None)
        q.cap = self.capacity if cap is None else int(cap)
        cand = np.zeros(max(q.cap, 1), np.int32)
        q.candidates = cand.ctypes.data
        keep = {}
        if taps:
            for name, dt in _KFDB_TAPS:
                keep[name] = np.zeros(self.capacity, dt)
                setattr(q, "tap_" + name, keep[name].ctypes.data)
        _check(lib().orbx_kfdb_query(self._ctx.handle, self._h, ctypes.byref(q)), "orbx_kfdb_query")
        info = dict(n_candidates=q.n_candidates, min_score_used=np.float32(q.min_score_used),
                    max_common_words=q.max_common_words, n_sharing=q.n_sharing, n_scored=q.n_scored)
        info.update(keep)
        return cand[:q.n_candidates].copy(), info

    def detect_relocalisation_candidates(self, query, taps=False, cap=None, info=False):
        """DetectRelocalisationCandidates(F): the candidate ids in the
        reference's order; with taps or info also a dict of the header
        (max_common_words, n_sharing, n_scored) and the per-id taps."""
        c, i = self._detect(KFDB_RELOC, query, 0.0, (), (), taps, cap)
        return (c, i) if (taps or info) else c

    def detect_loop_candidates(self, query, min_score=1.0, ref=(), exclude=(), taps=False, cap=None, info=False):
        """DetectLoop's minScore over `ref` (GetVectorCovisibleKeyFrames,
        starting at min_score) and DetectLoopCandidates with `exclude`
        (GetConnectedKeyFrames)."""
        c, i = self._detect(KFDB_LOOP, query, min_score, ref, exclude, taps, cap)
        return (c, i) if (taps or info) else c


class CovisReference(ctypes.Structure):
    """orbx_covis_reference_args (include/orbx.h)."""
    _fields_ = [("n", ctypes.c_int), ("frame_mp", ctypes.c_void_p), ("frame_erased", ctypes.c_void_p),
                ("local_kf", ctypes.c_void_p), ("kf_cap", ctypes.c_int), ("n_local_kf", ctypes.c_int),
                ("n_voters", ctypes.c_int), ("ref_kf", ctypes.c_int), ("local_mp", ctypes.c_void_p),
                ("mp_cap", ctypes.c_int), ("n_local_mp", ctypes.c_int)]


class CovisCull(ctypes.Structure):
    """orbx_covis_cull_args (include/orbx.h)."""
    _fields_ = [("cur", ctypes.c_int), ("n_keep", ctypes.c_int), ("keep", ctypes.c_void_p),
                ("max_culls", ctypes.c_int), ("cand_cap", ctypes.c_int), ("cand", ctypes.c_void_p),
                ("n_cand", ctypes.c_int), ("n_done", ctypes.c_int), ("n_mps", ctypes.c_void_p),
                ("n_redundant", ctypes.c_void_p), ("decision", ctypes.c_void_p), ("bad_points", ctypes.c_void_p),
                ("bad_cap", ctypes.c_int), ("n_bad", ctypes.c_int)]


COVIS_ORDERED, COVIS_ALL = 0, 1
COVIS_MAX_KEYFRAMES, COVIS_MAX_KEYPOINTS, COVIS_MAX_POINTS = 8192, 65535, 1 << 27


class CovisibilityMap:
    """The covisibility graph in HBM (orbx_covis_*): the keyframes' map-point
    rows and the connection weights, KeyFrame::UpdateConnections, the
    covisibility reads and Tracking::UpdateReference.  Keyframes and points
    are named by mnId; every keyframe carries a 64-bit order key that stands
    for its KeyFrame* value."""

    def __init__(self, ctx, kf_capacity, mp_capacity, max_keypoints):
        self._ctx = ctx
        self.kf_capacity, self.mp_capacity, self.max_keypoints = int(kf_capacity), int(mp_capacity), int(max_keypoints)
        self._h = ctypes.c_void_p()
        _check(lib().orbx_covis_create(ctx.handle, self.kf_capacity, self.mp_capacity, self.max_keypoints,
                                       ctypes.byref(self._h)), "orbx_covis_create")

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().orbx_covis_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return lib().orbx_covis_size(self._h)

    def clear(self):
        _check(lib().orbx_covis_clear(self._ctx.handle, self._h), "orbx_covis_clear")

    def add_keyframe(self, kf_id, key, mp):
        """A keyframe with its row mvpMapPoints (point ids or -1)."""
        mp = np.ascontiguousarray(mp, np.int32).reshape(-1)
        _check(lib().orbx_covis_add_keyframe(self._ctx.handle, self._h, int(kf_id), int(key), len(mp),
                                             _ptr(mp) if len(mp) else None), "orbx_covis_add_keyframe")

    def set_matches(self, kf_id, idx, mp):
        """row[idx[k]] = mp[k] in order; -1 erases the match."""
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        mp = np.ascontiguousarray(mp, np.int32).reshape(-1)
        if len(idx) != len(mp):
            raise ValueError("as many points as indices")
        _check(lib().orbx_covis_set_matches(self._ctx.handle, self._h, int(kf_id), len(idx), _ptr(idx) if len(idx) else None,
                                            _ptr(mp) if len(mp) else None), "orbx_covis_set_matches")

    def erase_points(self, ids):
        """MapPoint::SetBadFlag for every id."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        _check(lib().orbx_covis_erase_points(self._ctx.handle, self._h, len(ids), _ptr(ids) if len(ids) else None),
               "orbx_covis_erase_points")

    def erase_keyframe(self, kf_id):
        """The connection part of KeyFrame::SetBadFlag."""
        _check(lib().orbx_covis_erase_keyframe(self._ctx.handle, self._h, int(kf_id)), "orbx_covis_erase_keyframe")

    def update_connections(self, ids, th=15):
        """KeyFrame::UpdateConnections for `ids`, in order: (updated, front)."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        updated = np.zeros(max(len(ids), 1), np.int32)
        front = np.full(max(len(ids), 1), -1, np.int32)
        _check(lib().orbx_covis_update_connections(self._ctx.handle, self._h, len(ids), _ptr(ids) if len(ids) else None,
                                                   int(th), _ptr(updated), _ptr(front)), "orbx_covis_update_connections")
        return updated[:len(ids)], front[:len(ids)]

    def connections(self, kf_id, which=COVIS_ORDERED, cap=None):
        """(keyframes, weights): the ordered list (COVIS_ORDERED) or the whole
        row in ascending key order (COVIS_ALL)."""
        cap = self.kf_capacity if cap is None else int(cap)
        kfs, ws = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        n = ctypes.c_int()
        _check(lib().orbx_covis_connections(self._ctx.handle, self._h, int(kf_id), int(which), _ptr(kfs), _ptr(ws), cap,
                                            ctypes.byref(n)), "orbx_covis_connections")
        return kfs[:n.value].copy(), ws[:n.value].copy()

    def best_covisibility_keyframes(self, kf_id, n):
        """GetBestCovisibilityKeyFrames(n)."""
        return self.connections(kf_id)[0][:n]

    def update_reference(self, frame_mp, kf_cap=None, mp_cap=None):
        """Tracking::UpdateReferenceKeyFrames + UpdateReferencePoints: a dict
        of frame_erased, local_kf, n_voters, ref_kf and local_mp."""
        f = np.ascontiguousarray(frame_mp, np.int32).reshape(-1)
        q = CovisReference()
        q.n = len(f)
        er = np.zeros(max(len(f), 1), np.uint8)
        q.kf_cap = self.kf_capacity if kf_cap is None else int(kf_cap)
        q.mp_cap = min(self.mp_capacity, self.kf_capacity * self.max_keypoints) if mp_cap is None else int(mp_cap)
        lk, lm = np.zeros(max(q.kf_cap, 1), np.int32), np.zeros(max(q.mp_cap, 1), np.int32)
        q.frame_mp = f.ctypes.data if len(f) else None
        q.frame_erased, q.local_kf, q.local_mp = er.ctypes.data, lk.ctypes.data, lm.ctypes.data
        r = lib().orbx_covis_update_reference(self._ctx.handle, self._h, ctypes.byref(q))
        out = dict(frame_erased=er[:len(f)].copy(), n_local_kf=q.n_local_kf, n_voters=q.n_voters, ref_kf=q.ref_kf,
                   n_local_mp=q.n_local_mp, local_kf=lk[:min(q.n_local_kf, q.kf_cap)].copy(),
                   local_mp=lm[:min(q.n_local_mp, q.mp_cap)].copy(), code=r)
        if r != -3 or (kf_cap is None and mp_cap is None):   # with caps of the caller's, ORBX_ERR_CAPACITY is an answer
            _check(r, "orbx_covis_update_reference")
        return out

    def set_octaves(self, kf_id, octave):
        """mvKeysUn[i].octave of a member, as many as its row has entries."""
        o = np.ascontiguousarray(octave, np.uint8).reshape(-1)
        _check(lib().orbx_covis_set_octaves(self._ctx.handle, self._h, int(kf_id), len(o), _ptr(o) if len(o) else None),
               "orbx_covis_set_octaves")

    def cull_keyframes(self, cur=-1, keep=(), max_culls=0, cand=None, cand_cap=None, bad_cap=None):
        """LocalMapping::KeyFrameCulling over the ordered list of member `cur`,
        or over `cand` with cur = -1 (the form that resumes after max_culls):
        a dict of cand, n_done, n_mps, n_redundant, decision (-1 skipped, 0
        stays, 1 culled, 2 kept by `keep`) and bad_points."""
        keep = np.ascontiguousarray(keep, np.int32).reshape(-1)
        q = CovisCull()
        q.cur, q.max_culls = int(cur), int(max_culls)
        q.n_keep, q.keep = len(keep), (keep.ctypes.data if len(keep) else None)
        given = np.ascontiguousarray(cand if cand is not None else [], np.int32).reshape(-1)
        room = max(self.kf_capacity, len(given))
        q.cand_cap = room if cand_cap is None else int(cand_cap)
        q.bad_cap = min(self.mp_capacity, self.kf_capacity * self.max_keypoints) if bad_cap is None else int(bad_cap)
        size = max(q.cand_cap, len(given), 1)
        c, nm, nr, de = (np.zeros(size, np.int32) for _ in range(4))
        c[:len(given)] = given
        q.n_cand = len(given)
        bad = np.zeros(max(q.bad_cap, 1), np.int32)
        q.cand, q.n_mps, q.n_redundant, q.decision = c.ctypes.data, nm.ctypes.data, nr.ctypes.data, de.ctypes.data
        q.bad_points = bad.ctypes.data
        r = lib().orbx_covis_cull_keyframes(self._ctx.handle, self._h, ctypes.byref(q))
        if r != -3 or (cand_cap is None and bad_cap is None):   # with caps of the caller's, ORBX_ERR_CAPACITY is an answer
            _check(r, "orbx_covis_cull_keyframes")
        nd = min(q.n_done, q.cand_cap)
        return dict(code=r, n_cand=q.n_cand, n_done=q.n_done, n_bad=q.n_bad, cand=c[:min(q.n_cand, max(q.cand_cap, len(given)))].copy(),
                    n_mps=nm[:nd].copy(), n_redundant=nr[:nd].copy(), decision=de[:nd].copy(),
                    bad_points=bad[:min(q.n_bad, q.bad_cap)].copy())

    def cull_points(self, cur_kf, ids, found, visible, first_kf):
        """LocalMapping::MapPointCulling over mlpRecentAddedMapPoints = ids:
        the action per point (0 keep, 1 erased already, 2 found ratio, 3 two
        observers or fewer, 4 old enough to leave the list)."""
        a = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in (ids, found, visible, first_kf)]
        n = len(a[0])
        if any(len(x) != n for x in a):
            raise ValueError("one entry per point in every array")
        action = np.zeros(max(n, 1), np.int32)
        ptrs = [x.ctypes.data if n else None for x in a]
        _check(lib().orbx_covis_cull_points(self._ctx.handle, self._h, int(cur_kf), n, *ptrs, action.ctypes.data),
               "orbx_covis_cull_points")
        return action[:n]


def describe_levels(w, h, nfeatures=1000, scale_factor=1.2, nlevels=8, fast_th=20):
    """Per-level host tables of the extractor (no device needed): list of
    dicts {w, h, n_desired, cols, rows, nfeatures_cell, n_cells, n_valid}."""
    out = np.zeros(8 * nlevels, np.int32)
    n = lib().orbx_describe_levels(nfeatures, scale_factor, nlevels, fast_th, w, h, _ptr(out), out.size)
    _check(0 if n > 0 else n, "orbx_describe_levels")
    keys = ["w", "h", "n_desired", "cols", "rows", "nfeatures_cell", "n_cells", "n_valid"]
    return [dict(zip(keys, map(int, out[8 * l:8 * l + 8]))) for l in range(n)]


def frame_view(kps, desc, w, h, nlevels=8, scale_factor=1.2):
    """orbx_frame_view over numpy keypoints/descriptors (Frame without
    distortion: bounds 0..w, 0..h, src/Frame.cc:341-347).  Keep the arrays
    alive while the view is used."""
    v = FrameView()
    v.keys_un = kps.ctypes.data
    v.desc = desc.ctypes.data
    v.n = len(kps)
    v.min_x, v.max_x, v.min_y, v.max_y = 0.0, float(w), 0.0, float(h)
    v.nlevels = nlevels
    v.scale_factor = scale_factor
    return v
