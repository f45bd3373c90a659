"""Timing of ``gmb_append`` against its yardstick on the same commit: ``gmb_set_data + gmb_set_theta + gmb_factorize`` at N + K --
what absorbing K new observations cost before the bordered update existed.

    python tools/gpu_append.py          N = 10,000 d = 4 ExpQuad;  K = 1, 16 and 128

Per K, behind ``factorize`` at N (median of ``REPEATS`` appends, the engine truncated back to N in between):

* the HIP-event time of the update (``kbuild_ms`` = the rebuilt rows of Sigma, ``chol_ms`` = panel solve + corner update + corner
  factorisation + v) against the same two phases of the fresh factorisation, and both calls' wall time on the host (the fresh
  route's includes its copies of X and y and the preparation of all points);
* where the update's time goes, from the engine's profiling log (``gmb_set_profiling`` + ``GMB_TRACE_FILE``): launch kinds
  2 = the panel solve's products, 5 = strip solves (panel and corner), 16 = the split-k corner update, 1 = the corner's leaves,
  0 = the corner's own trailing products.

Then the split-k launch pair (kind 16) against ``gmb_blk_gemm_nt`` (kind 0: ONE workgroup for the tile) on the corner's shape at
this N: m = n = 128, k = 9984, alpha = -1, beta = 1.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``GA_TIMEOUT`` seconds,
default 300), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, KIND = 10_000, 4, "ExpQuad"
KS = (1, 16, 128)
REPEATS = 5
KINDS = {2: "panel products", 5: "strip solves", 16: "split-k corner update", 1: "corner leaves", 0: "corner products"}


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from gumbi_amd.engine import Engine, KernelSpec
    from oracle import gp_oracle as O

    trace = os.environ["GMB_TRACE_FILE"]
    X, y, ls = O.synthetic_table(N + max(KS), D)
    spec = O.make_spec(D, range(D), kind=KIND)
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    kspec = KernelSpec(D=D, idx_cont=list(range(D)), kind=KIND)

    def events():  # {kind: [ms, ...]} logged since the last call
        out = {}
        with open(trace) as fh:
            for line in fh:
                f = line.split()
                out.setdefault(int(f[0]), []).append(float(f[5]))
        open(trace, "w").close()
        return out

    def phases(eng):
        tm = eng.timings()
        return tm["kbuild_ms"], tm["chol_ms"]

    print(f"N={N} d={D} {KIND}; median of {REPEATS}")
    with Engine(0) as eng, Engine(0) as fresh:
        eng.set_data(X[:N], y[:N])
        eng.set_kernel(kspec)
        eng.set_theta(theta)
        eng.factorize()
        fresh.set_kernel(kspec)
        for K in KS:
            Xn, yn = X[N:N + K], y[N:N + K]
            eng.append(Xn, yn)  # allocations, code objects
            eng.truncate(N)
            t_dev, t_wall, f_dev, f_wall = [], [], [], []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                eng.append(Xn, yn)
                t_wall.append(1e3 * (time.perf_counter() - t0))
                t_dev.append(phases(eng))
                v1 = eng.copy_v()
                eng.truncate(N)
                t0 = time.perf_counter()
                fresh.set_data(X[:N + K], y[:N + K])
                fresh.set_theta(theta)
                fresh.factorize()
                f_wall.append(1e3 * (time.perf_counter() - t0))
                f_dev.append(phases(fresh))
            eng.set_profiling(True)
            events()
            eng.append(Xn, yn)
            ev = events()
            eng.set_profiling(False)
            v2 = eng.copy_v()
            eng.truncate(N)
            a_k, a_c = np.median(np.array(t_dev), axis=0)
            f_k, f_c = np.median(np.array(f_dev), axis=0)
            print(f"  K={K:4d}: gmb_append   device {a_k + a_c:8.3f} ms (Sigma rows {a_k:.3f} + update {a_c:.3f})   wall {np.median(t_wall):8.3f} ms")
            print(f"          fresh at N+K device {f_k + f_c:8.3f} ms (K-build {f_k:.3f} + Cholesky {f_c:.3f})   wall {np.median(f_wall):8.3f} ms"
                  f"   ratio device {(f_k + f_c) / (a_k + a_c):.1f}x wall {np.median(f_wall) / np.median(t_wall):.1f}x")
            print("          while profiling: " + ", ".join(f"{KINDS[k]} {sum(ev.get(k, [])):.3f} ms ({len(ev.get(k, []))})" for k in KINDS))
            print(f"          same bits call after call: {v1.tobytes() == v2.tobytes()}", flush=True)

        # the corner update's launch pair against one workgroup per tile, on caller-provided blocks
        m, k = 128, (N // 128) * 128
        dev = torch.device("cuda:0")
        g = torch.Generator(device="cpu").manual_seed(0)
        tA = torch.randn((k, m), dtype=torch.float64, generator=g).to(dev)
        tC = torch.randn((m, m), dtype=torch.float64, generator=g).to(dev)
        torch.cuda.synchronize()
        Xs = X[:16]
        eng.set_profiling(True)
        events()
        S = 0
        for _ in range(REPEATS + 1):
            S = eng.blk_gemm_splitk(tC.data_ptr(), m, tA.data_ptr(), m, tA.data_ptr(), m, m, m, k, -1.0, 1.0, 0)
            eng.blk_gemm_nt(tC.data_ptr(), m, tA.data_ptr(), m, tA.data_ptr(), m, m, m, k, -1.0, 1.0)
        eng.predict(Xs)  # (synchronises the engine's stream and collects the events)
        ev = events()
        eng.set_profiling(False)
        sk, one = np.median(ev[16][1:]), np.median(ev[0][1:])
        gf = 2.0 * m * m * k / 1e9
        print(f"  corner update m = n = {m}, k = {k}: split-k pair ({S} slices) {1e3 * sk:8.1f} us ({gf / sk:.0f} GF/s)   "
              f"gmb_blk_gemm_nt {1e3 * one:8.1f} us ({gf / one:.0f} GF/s)   ratio {one / sk:.1f}x", flush=True)


def main():
    limit = os.environ.get("GA_TIMEOUT", "300")
    with tempfile.NamedTemporaryFile(prefix="append_trace_", suffix=".txt") as tf:
        env = dict(os.environ, GMB_TRACE_FILE=tf.name)
        rc = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode
    if rc != 0:
        print(f"the child ended with status {rc}; nothing further is started")
    return rc


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main())
