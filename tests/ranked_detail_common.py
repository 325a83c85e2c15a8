"""TEST INFRASTRUCTURE shared by test_emu_ranked_detail.py / test_gpu_ranked_detail.py: the reference values of a
cc_ranked_detail_t from the CPU oracle, and the structural properties every detail answer has.

For an entry with ranked row e (scan, correlation, pose) and detail row d, src = the candidate's scan, tgt = the query's:
  * oracle.gmm(src, tgt, d.tf_init) must give d.corr_init, e.correlation, e.tf within TOL and (d.iterations, d.termination) exactly;
  * grad: the oracle's analytic gradient at e.tf over the pair set of d.tf_init, divided by nrm = sqrt(ac_src ac_tgt);
    bar 1e-10 sqrt(H_kk) absolute (both sides are f64 sums of <~ 2 000 terms of <~ 1e-2: reassociation moves them by ~1e-15,
    ~1e-13 on theta with its ~100 px lever arm; one wrong pair or a pose off by 1e-6 gives H dp ~ 1e-8);
  * hess: the five-point central difference of that gradient at e.tf, steps (5e-3, 5e-3, 5e-5) and half of them.  The two
    step sizes must agree within 1e-9 in the metric |dH_ij| / sqrt(H_ii H_jj) (measured spread 1.5e-11), else the test fails;
    the device must be within 1e-8 of the half-step reference in the same metric (500 x the reference's spread, four orders
    below what a missing or mis-signed term of the closed form produces)."""
import numpy as np

from ranked_common import TOL

STEPS = np.array([5e-3, 5e-3, 5e-5])
REF_AGREE = 1e-9   # the reference's two step sizes, scaled metric
HESS_BAR = 1e-8    # device against the half-step reference, scaled metric
GRAD_BAR = 1e-10   # x sqrt(H_kk), absolute
CONVERGED = (1, 2, 3)
_scans = {}


def scan_of(oracle, desc, i, key):
    k = (key, int(i))
    if k not in _scans:
        _scans[k] = oracle.Scan.from_desc(desc[int(i)], int_id=int(i))
    return _scans[k]


def mat(h6):
    h = np.asarray(h6, np.float64)
    return np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])


def ref_hessian(G, p, steps):
    """five-point central difference of the gradient function G at p, symmetrised"""
    H = np.zeros((3, 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = steps[k]
        H[:, k] = (-G(p + 2 * e) + 8 * G(p + e) - 8 * G(p - e) + G(p - 2 * e)) / (12 * steps[k])
    return 0.5 * (H + H.T)


def scaled(dH, H):
    s = np.sqrt(np.abs(np.diag(H)))
    return float(np.abs(dH / np.outer(s, s)).max())


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


def check_entry(oracle, src, tgt, e, d, what, stats):
    """every reference comparison of one listed entry; the observed figures are gathered in stats (dict of lists)"""
    tf_init = np.array(d["tf_init"], np.float64)
    p = np.array(e["tf"], np.float64)
    ci, co, tf, it = oracle.gmm(src, tgt, tf_init)
    dtf = tf - p
    dtf[2] = wrap(dtf[2])
    stats["corr_init"].append(abs(ci - d["corr_init"]))
    stats["corr"].append(abs(co - e["correlation"]))
    stats["tf"].append(float(np.abs(dtf).max()))
    assert abs(ci - d["corr_init"]) < TOL, (what, ci, d["corr_init"])
    assert abs(co - e["correlation"]) < TOL, (what, co, e["correlation"])
    assert np.abs(dtf).max() < TOL, (what, tf, p)
    assert (int(it[0]), int(it[1])) == (int(d["iterations"]), int(d["termination"])), (what, it, d["iterations"], d["termination"])
    _, g0, ac = oracle.gmm_eval(src, tgt, tf_init, p)
    nrm = np.sqrt(ac[0] * ac[1])
    G = lambda x: oracle.gmm_eval(src, tgt, tf_init, x)[1] / nrm  # noqa: E731
    H = mat(d["hess"])
    gerr = np.abs(g0 / nrm - d["grad"]) / np.sqrt(np.abs(np.diag(H)))
    stats["grad"].append(float(gerr.max()))
    H1 = ref_hessian(G, p, STEPS)
    H2 = ref_hessian(G, p, STEPS / 2)
    agree = scaled(H1 - H2, H2)
    herr = scaled(H - H2, H2)
    stats["ref_agree"].append(agree)
    stats["hess"].append(herr)
    ev = np.linalg.eigvalsh(H)
    if int(d["termination"]) in CONVERGED:
        stats["min_eig"].append(float(ev[0]))
    print("%s n_pairs %d it %d term %d: grad %.2e (x sqrt Hkk) ref-agree %.2e hess %.2e min-eig %.3e" %
          (what, d["n_pairs"], d["iterations"], d["termination"], gerr.max(), agree, herr, ev[0]))
    assert (gerr < GRAD_BAR).all(), (what, "grad", g0 / nrm, d["grad"], gerr)
    assert agree < REF_AGREE, (what, "the reference's two step sizes disagree", agree)
    assert herr < HESS_BAR, (what, "hess", H, H2, herr)
    if int(d["termination"]) in CONVERGED:
        assert ev[0] > 0, (what, "not positive definite at a converged optimum", ev)


def new_stats():
    return {k: [] for k in ("corr_init", "corr", "tf", "grad", "ref_agree", "hess", "min_eig")}


def report(stats, what):
    print("%s: %d entries; max |corr_init| %.2e |corr| %.2e |tf| %.2e; grad %.2e (x sqrt Hkk); reference agreement %.2e; hess %.2e; "
          "smallest eigenvalue at a converged entry %.3e" % (what, len(stats["hess"]), max(stats["corr_init"]), max(stats["corr"]), max(stats["tf"]),
                                                             max(stats["grad"]), max(stats["ref_agree"]), max(stats["hess"]),
                                                             min(stats["min_eig"]) if stats["min_eig"] else float("nan")))


def check_rows(oracle, desc, key, q_of_row, cands, cnt, det, what, stats, rows=None, max_entries=None):
    """the reference comparisons on every listed entry of the given rows (all rows by default); -> entries checked"""
    n = 0
    for i in (range(len(cands)) if rows is None else rows):
        tgt = scan_of(oracle, desc, q_of_row[i], key)
        for k in range(int(cnt[i])):
            if max_entries is not None and n >= max_entries:
                return n
            e, d = cands[i][k], det[i][k]
            src = scan_of(oracle, desc, e["cand_gidx"], key)
            check_entry(oracle, src, tgt, e, d, (what, int(q_of_row[i]), k, int(e["cand_gidx"])), stats)
            n += 1
    return n


def check_structure(L, cands, cnt, det, max_ret):
    """rows beyond h_n are zero bytes; flags equal the ranked entry's; the six numbers are a symmetric matrix by construction"""
    assert det.shape == cands.shape == (len(cnt), max_ret) and det.dtype == L.ranked_detail_dt
    zero = np.zeros(1, L.ranked_detail_dt).tobytes()
    for i in range(len(cnt)):
        for k in range(max_ret):
            if k < cnt[i]:
                assert det[i][k]["flags"] == cands[i][k]["flags"], (i, k)
                assert det[i][k]["n_pairs"] > 0 and 0 <= det[i][k]["iterations"] <= 10, (i, k, det[i][k])
                H = mat(det[i][k]["hess"])
                assert np.array_equal(H, H.T) and np.isfinite(H).all() and np.isfinite(det[i][k]["grad"]).all()
            else:
                assert det[i][k].tobytes() == zero, (i, k, det[i][k])
