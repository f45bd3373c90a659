"""Timing of ``gmb_loo`` / ``gmb_leave_out`` behind a fit's last evaluation, against what a refit-free user would compare them
with on the same commit: one ``gmb_factorize`` and one ``gmb_predict`` of M = N points.

    python tools/gpu_leave_out.py          the benchmark's N = 10,000 table (d = 4, ExpQuad-ARD: bench.py's C2)

Behind ``evaluate(theta, grad=True)`` (the tile path: U = L^-T and alpha resident).  Every time is the HIP-event time of the call
on the engine's stream (``predict_ms`` of ``gmb_timings``; ``chol_ms + kbuild_ms`` for the factorisation), medians of ``REPEATS``
calls after a warm-up of each, profiling off.  Timed:

* ``gmb_loo``, product form: its time, and the 4 N^2 bytes of the triangle it must read over that time, against the 6.29 TB/s a
  device-to-device copy reaches on this part;
* ``gmb_loo``, solve form (``gmb_set_predict_form(e, 0)``);
* ``gmb_leave_out`` for m = 128, 1024 and 2000 rows (every (N / m)-th row), with and without ``cov``;
* ``gmb_factorize`` and ``gmb_predict`` at M = N -- the factorisation is timed LAST: it ends the residency of U.

The claim to support or retract: a leave-one-out sweep behind a fit costs less than one factorisation.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 300), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 10_000, 4
REPEATS = 5
COPY_TBS = 6.29
GROUPS = (128, 1024, 2000)


def child():
    sys.path.insert(0, ROOT)
    import numpy as np

    from gumbi_amd.engine import Engine, KernelSpec
    from oracle import gp_oracle as O

    X, y, ls = O.synthetic_table(N, D)
    spec = O.make_spec(D, range(D), kind="ExpQuad")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)

    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=True, jitter=spec["jitter"]))
        eng.evaluate(theta, grad=True)

        def timed(call):
            call()  # allocations, code objects
            ms, out = [], None
            for _ in range(REPEATS):
                out = call()
                ms.append(eng.timings()["predict_ms"])
            return float(np.median(ms)), min(ms), max(ms), out

        def line(label, t, extra=""):
            print(f"  {label:<44s} {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}){extra}", flush=True)

        print(f"N={N} d={D} ExpQuad-ARD, behind evaluate(theta, grad=True); medians of {REPEATS} calls after a warm-up")
        eng.predict(X[:256])
        assert eng.timings()["predict_gemm_form"] == 1, "U is not resident: the evaluation did not take the tile path"
        prod = timed(lambda: eng.loo())
        tri_bytes = 4.0 * N * N
        rate = tri_bytes / (prod[0] * 1e-3) / 1e12
        line("gmb_loo, product form (all N rows)", prod, f"   {tri_bytes / 1e9:.3f} GB of U = {rate:.2f} TB/s = {rate / COPY_TBS:.2f} of the copy rate")
        eng.set_predict_form(0)
        solve = timed(lambda: eng.loo())
        eng.set_predict_form(-1)
        line("gmb_loo, solve form (all N rows)", solve)
        err_m = float(np.max(np.abs(prod[3][0] - solve[3][0])) / np.max(np.abs(solve[3][0])))
        err_v = float(np.max(np.abs(prod[3][1] - solve[3][1])))
        print(f"    product against solve: mean {err_m:.2e} relative, variance {err_v:.2e} absolute")
        for m in GROUPS:
            rows = np.arange(0, N, N // m)[:m]
            line(f"gmb_leave_out, m = {m}", timed(lambda: eng.leave_out(rows)))
            line(f"gmb_leave_out, m = {m}, with cov", timed(lambda: eng.leave_out(rows, cov=True)))
        line(f"gmb_predict, M = N = {N} (product form)", timed(lambda: eng.predict(X)))

        def factorize():
            eng.factorize()
            tm = eng.timings()
            return tm["kbuild_ms"] + tm["chol_ms"]

        factorize()
        fac = [factorize() for _ in range(REPEATS)]
        fac_ms = float(np.median(fac))
        print(f"  {'gmb_factorize (K build + Cholesky)':<44s} {fac_ms:9.3f} ms  (min {min(fac):.3f}, max {max(fac):.3f})")
        line(f"gmb_predict, M = N = {N} (solve form)", timed(lambda: eng.predict(X)))
        line("gmb_loo, solve form behind gmb_factorize", timed(lambda: eng.loo()))
        print(f"  a leave-one-out sweep behind the fit / one factorisation: product form {prod[0] / fac_ms:.3f}, solve form {solve[0] / fac_ms:.3f}",
              flush=True)


def main():
    limit = os.environ.get("TC_TIMEOUT", "300")
    rc = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--child"]).returncode
    if rc != 0:
        print(f"the child ended with status {rc}; nothing further is started")
    return rc


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main())
