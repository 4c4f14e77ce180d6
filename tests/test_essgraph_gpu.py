"""Optimizer::OptimizeEssentialGraph on the device
(orbx_optimize_essential_graph) against the numpy restatement
tests/essgraph_numpy.py, in two layers like tests/test_sim3opt_gpu.py.

Layer 1, each step fed the DEVICE's own tapped state:
* the measurements byte for byte (+ - * / and sqrt only);
* the per-edge errors and Jacobians at the first iteration, and for every
  iteration the device ran the restatement's chi2, b and diagonal blocks at the
  device's it_est, within the measured bars (essgraph_numpy.TOL);
* the last trial's dx of every iteration against the restatement's own solve of
  the device-consistent system (its H and b at the device's it_est, the
  device's lambda of that trial);
* Tcw_out and the corrected points byte for byte from the device's est_out:
  only + - * / and casts separate them.

Layer 2, end to end against the restatement's own run: the iteration count and
the per-iteration trial counts over the decisive iterations (the restatement's
gain (ini - cur) / ini >= 1e-3, the stop rule's own threshold; the others turn
on rounding and are printed), est_out (sign-aligned), chi2_last, Tcw_out and
pos_out.  An iteration that accepts nothing leaves the estimates equal to its
it_est, byte for byte.

The bars are measured, not chosen: essgraph_numpy.MEASURED x 8 (DESIGN.md
section 4); tests/test_essgraph_numpy.py asserts that the measurement
reproduces.  Every compared figure is printed before it is asserted.
"""
import ctypes

import numpy as np
import pytest

import essgraph_numpy as en
import orb_slam_amd as ox

pytestmark = pytest.mark.gpu
TOL = en.TOL
NAMES = [n for n in en.CASES if n != "floating"]


@pytest.fixture(scope="module")
def ctx():
    c = ox.Context(nfeatures=500, max_w=160, max_h=120, slots=1)
    yield c
    c.close()


def arrays(g):
    return ox.essgraph_arrays(g["ids"], g["Tcw"], g["edges"], g["corrected"], g["noncorrected"])


def run(ctx, g, taps=True):
    kfs, edges = arrays(g)
    return ctx.optimize_essential_graph(kfs, edges, g["loop_kf"], g["cur_kf"], pos=g["pos"], ref_kf=g["ref_kf"], taps=taps)


_runs = {}


def device(ctx, name):
    """One tapped device run per case, shared by the tests."""
    if name not in _runs:
        _runs[name] = run(ctx, en.case(name)[0])
    return _runs[name]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def held(what, name, value, bar):
    print(f"{name}: {what} {value:.3e} (bar {bar:.3e})")
    return value <= bar


def lambdas_of(d):
    """lambda before the last trial of each iteration: the iteration starts
    from the previous one's final lambda and multiplies it by 2, 4, 8, ...
    over its rejected trials."""
    out, lam = [], en.LAMBDA_INIT
    for k in range(d["iterations"]):
        ni = 2.0
        for _ in range(d["it_trials"][k] - 1):
            lam *= ni
            ni *= 2
        out.append(lam)
        lam = d["it_lambda"][k]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_layer1_every_step_from_the_device_state(ctx, name):
    g, ref = en.case(name)
    d = device(ctx, name)
    pl = en.plan(g["ids"], g["loop_kf"], g["edges"])
    assert (d["n_free"], d["n_blocks"], d["max_row_blocks"]) == (pl["n_free"], pl["n_blocks"], pl["max_row_blocks"])
    vscw, meas = en.setup(g)
    assert bits(d["edge_meas"]) == bits(meas)
    assert d["iterations"] >= 1 and d["trials"] == int(d["it_trials"].sum())
    assert bits(d["it_est"][0]) == bits(vscw)
    ok = True
    lam = lambdas_of(d)
    nf = pl["n_free"]
    for k in range(d["iterations"]):
        chi, H, b, err, J, _ = en.linearize(g, meas, d["it_est"][k], pl)
        if k == 0:
            ok &= held("edge error", name, en.rel(err, d["edge_err"]), TOL["err"])
            ok &= held("edge J", name, en.rel(J.reshape(len(err), 98), d["edge_J"]), TOL["J"])
            assert d["chi2_first"] == d["it_chi2"][0]
        ok &= held(f"it {k} chi2", name, en.rel(chi, d["it_chi2"][k]), TOL["chi2"])
        ok &= held(f"it {k} b", name, en.rel(b, d["it_b"][k]), TOL["b"])
        ok &= held(f"it {k} Hdiag", name, en.rel(en.hdiag(H, nf), d["it_Hdiag"][k]), TOL["Hdiag"])
        solved, dx = en.cholesky_solve(H + lam[k] * np.eye(7 * nf), b)
        if solved and np.any(d["it_dx"][k] != 0):
            ok &= held(f"it {k} dx", name, en.rel(dx, d["it_dx"][k]), TOL["dx"])
    Tcw, swc = en.recover(d["est"])
    assert bits(d["Tcw"]) == bits(Tcw)
    assert bits(d["pos"]) == bits(en.correct_points(vscw, swc, g["pos"], g["ref_kf"]))
    assert ok


@pytest.mark.parametrize("name", NAMES)
def test_layer2_end_to_end(ctx, name):
    g, ref = en.case(name)
    d = device(ctx, name)
    decisive = [k for k, rec in enumerate(ref["log"]) if rec["gain"] >= 1e-3]
    print(f"{name}: iterations {d['iterations']} / {ref['iterations']}, trials {list(d['it_trials'])} / "
          f"{[r['trials'] for r in ref['log']]}, decisive {decisive}, not_posdef {d['not_posdef']}")
    for k in decisive:
        assert d["iterations"] > k and d["it_trials"][k] == ref["log"][k]["trials"]
    if len(decisive) == len(ref["log"]):
        assert d["iterations"] == ref["iterations"]
    ok = held("est", name, en.rel(ref["est"], en.align(d["est"], ref["est"])), TOL["est"])
    ok &= held("chi2_last", name, en.rel(ref["chi2_last"], d["chi2_last"]), TOL["chi2_last"])
    ok &= held("Tcw", name, en.rel(ref["Tcw"], d["Tcw"]), TOL["est"] + 2.0 ** -23)
    ok &= held("pos", name, en.rel(ref["pos"], d["pos"]), 16 * (TOL["est"] + 2.0 ** -23))
    # an iteration that accepts nothing leaves the estimates as they were
    est_after = [d["it_est"][k + 1] for k in range(d["iterations"] - 1)] + [d["est"]]
    for k in range(d["iterations"]):
        if k + 1 < d["iterations"] and d["it_chi2"][k + 1] == d["it_chi2"][k] or d["it_trials"][k] == en.MAX_TRIALS:
            assert bits(est_after[k]) == bits(d["it_est"][k])
    assert d["chi2_last"] <= d["chi2_first"]
    if name == "chain5_consistent":
        assert d["chi2_first"] == 0.0 and d["iterations"] == 1 and d["trials"] == 1
        assert bits(d["Tcw"]) == bits(g["Tcw"])
    if name == "hub130":       # the keyframe without an edge keeps its estimate
        lone = int(np.nonzero(en.plan(g["ids"], g["loop_kf"], g["edges"])["free_index"] < 0)[0][-1])
        assert lone != g["loop_kf"] and bits(d["est"][lone]) == bits(ref["vscw"][lone])
    assert ok


def test_floating_component_invariants(ctx):
    """A component joined to nothing fixed: H is singular up to lambda = 1e-16 and
    the reference's outcome is undefined, so only invariants hold: every output
    finite, chi2 not increased, and the connected component's result that of the
    same graph without the floating pair."""
    g, _ = en.case("floating")
    d = run(ctx, g)
    base = device(ctx, "loop12")
    print(f"floating: iterations {d['iterations']}, trials {list(d['it_trials'])}, not_posdef {d['not_posdef']}, "
          f"chi2 {d['chi2_first']} -> {d['chi2_last']}")
    assert np.all(np.isfinite(d["est"])) and np.all(np.isfinite(d["Tcw"]))
    assert np.isfinite(d["chi2_last"]) and d["chi2_last"] <= d["chi2_first"]
    n = len(base["est"])
    assert held("connected component", "floating", en.rel(base["est"], en.align(d["est"][:n], base["est"])), TOL["est"])


def test_two_runs_are_byte_equal_with_and_without_taps_and_timing(ctx):
    for name in ("loop13_gap", "hub130", "points"):
        g, _ = en.case(name)
        a, b, c = device(ctx, name), run(ctx, g), run(ctx, g, taps=False)
        ctx.timing(True)
        try:
            t = run(ctx, g, taps=False)
        finally:
            ctx.timing(False)
        for key in a:
            assert bits(a[key]) == bits(b[key]), key
        for key in c:
            assert bits(a[key]) == bits(c[key]) == bits(t[key]), key


def test_permuting_the_keyframes_changes_only_the_output_order(ctx):
    g, _ = en.case("loop13_gap")
    d = device(ctx, "loop13_gap")
    n = len(g["ids"])
    perm = np.random.RandomState(3).permutation(n)           # new position k holds old keyframe perm[k]
    at = np.argsort(perm)
    e = g["edges"].copy()
    e[:, 0], e[:, 1] = at[e[:, 0]], at[e[:, 1]]
    h = en.graph(g["ids"][perm], g["Tcw"][perm], e, at[g["loop_kf"]], at[g["cur_kf"]],
                 {at[k]: v for k, v in g["corrected"].items()}, {at[k]: v for k, v in g["noncorrected"].items()})
    p = run(ctx, h)
    assert bits(p["est"]) == bits(d["est"][perm]) and bits(p["Tcw"]) == bits(d["Tcw"][perm])
    assert p["iterations"] == d["iterations"] and bits(p["it_trials"]) == bits(d["it_trials"])
    assert bits(p["it_chi2"]) == bits(d["it_chi2"]) and bits(p["it_dx"]) == bits(d["it_dx"])


def test_no_edge_runs_recovery_and_points(ctx):
    g, _ = en.case("points")
    h = dict(g, edges=np.zeros((0, 3), np.int64))
    d = run(ctx, h)
    assert d["iterations"] == 0 and d["trials"] == 0 and d["n_free"] == 0
    vscw, _ = en.setup(h)
    Tcw, swc = en.recover(vscw)
    assert bits(d["est"]) == bits(vscw) and bits(d["Tcw"]) == bits(Tcw)
    assert bits(d["pos"]) == bits(en.correct_points(vscw, swc, g["pos"], g["ref_kf"]))


def test_refused_calls_leave_every_array_untouched(ctx):
    g, _ = en.case("points")

    def refused(code, mutate):
        kfs, edges = arrays(g)
        q, keep = ox.essgraph_query(kfs, edges, g["loop_kf"], g["cur_kf"], pos=g["pos"], ref_kf=g["ref_kf"], taps=True)
        mutate(q, keep)
        before = {k: bits(v) for k, v in keep.items()}
        assert ox.lib().orbx_optimize_essential_graph(ctx._h, ctypes.byref(q)) == code
        assert before == {k: bits(v) for k, v in keep.items()}

    def field(name, value):
        return lambda q, keep: setattr(q, name, value)

    def cell(array, index, name, value):
        def f(q, keep):
            keep[array][name][index] = value
        return f
    ARG, UNSUPPORTED = -1, -4
    refused(ARG, field("kfs", None))
    refused(ARG, field("Tcw_out", None))
    refused(ARG, field("pos_out", None))
    refused(ARG, field("n_kf", 0))
    refused(ARG, field("n_edges", -1))
    refused(ARG, field("n_points", -1))
    refused(ARG, field("loop_kf", 12))
    refused(ARG, field("cur_kf", -1))
    refused(ARG, cell("edges", 2, "i", 12))
    refused(ARG, cell("edges", 2, "j", -1))
    refused(ARG, cell("edges", 4, "j", int(arrays(g)[1]["i"][4])))
    refused(ARG, cell("edges", 0, "kind", 2))
    refused(ARG, cell("kfs", 5, "id", int(g["ids"][6])))
    refused(ARG, cell("kfs", 1, "Tcw", np.nan))
    refused(ARG, cell("kfs", g["cur_kf"], "corrected", np.inf))

    def zero_scale(q, keep):
        keep["kfs"]["noncorrected"][g["cur_kf"]][7] = 0.0
    refused(ARG, zero_scale)

    def bad_ref(q, keep):
        keep["ref_kf"][3] = 12
    refused(ARG, bad_ref)
    refused(UNSUPPORTED, field("n_kf", 16385))
    assert ox.lib().orbx_optimize_essential_graph(ctx._h, None) == ARG
    assert ox.lib().orbx_optimize_essential_graph(None, None) == ARG


def test_the_caps_admit_4096_keyframes_with_16_edges_each(ctx):
    """The documented caps pass 4096 keyframes with 16 edges each; one call's
    time is printed (no bar)."""
    import time
    n = 4096
    Tcw = np.array([np.concatenate([np.eye(3).reshape(9), [0.5 * (k % 64), 0.25 * (k // 64), 0.0]]) for k in range(n)],
                   np.float32)
    edges = [(k, k - d, 1) for k in range(n) for d in range(1, 17) if k - d >= 0]
    kfs, ed = ox.essgraph_arrays(np.arange(n), Tcw, edges)
    t = time.perf_counter()
    d = ctx.optimize_essential_graph(kfs, ed, 0, n - 1)
    print(f"4096 keyframes, {len(edges)} edges, consistent: {time.perf_counter() - t:.3f} s, "
          f"{d['iterations']} iteration(s), {d['trials']} trial(s), n_blocks {d['n_blocks']}")
    assert d["n_free"] == n - 1 and d["chi2_first"] == 0.0 and d["iterations"] == 1
    assert bits(d["Tcw"]) == bits(Tcw)


def test_timer_counts_one_region_per_call(ctx):
    g, _ = en.case("loop12")
    ctx.timing(True)
    try:
        ctx.kernel_time("essgraph")      # drains what earlier tests left
        run(ctx, g, taps=False)
        run(ctx, g, taps=False)
        n, avg, tot = ctx.kernel_time("essgraph")
        print(f"essgraph: {avg:.3f} ms per call over {n} calls")
        assert n == 2 and tot > 0
        for region in ("essgraph.linearize", "essgraph.factor", "essgraph.points"):
            assert ctx.kernel_time(region)[0] >= 2
    finally:
        ctx.timing(False)
