"""The engine's byte ledger (``gmb_resident_bytes``) along one fixed script of calls, on the MI355X.  Needs a GPU (``-m gpu``).

The ledger is the sum of the sizes the engine asked the device for -- exact integers -- so WHEN a buffer is allocated, grown,
marked stale or freed shows in it call by call.  ``tests/golden/resident_ledger.json`` holds ``(resident, peak)`` after every
step of ``ledger_script``; the test asserts equality, without a tolerance.  A change that moves a number on purpose (a new
workspace, another size rule) re-records the file and says so:

    python tests/test_gpu_resident_ledger.py tests/golden/resident_ledger.json
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "resident_ledger.json"
D = 3


def ledger_script():
    """``[[step, resident, peak], ...]`` of the script below on device 0."""
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    from gumbi_amd.engine import Engine, KernelSpec
    from oracle import gp_oracle as O

    X, y, ls = O.synthetic_table(401, D)  # rows [0, 300) the first data set, [300, 401) the appended ones
    spec = O.make_spec(D, range(D), kind="ExpQuad")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    rng = np.random.default_rng(7)
    Xs200, Xs150 = rng.standard_normal((200, D)), rng.standard_normal((150, D))
    Z = rng.standard_normal((4, 150))
    kernel = KernelSpec(D=D, idx_cont=list(range(D)), kind="ExpQuad")
    out = []

    def step(eng, name, call):
        call()
        out.append([name, eng.resident_bytes(), eng.resident_bytes(peak=True)])

    with Engine(0) as eng:
        step(eng, "create", lambda: None)
        step(eng, "set_data N=300", lambda: eng.set_data(X[:300], y[:300]))  # three block columns, the last one ragged
        step(eng, "set_kernel", lambda: eng.set_kernel(kernel))
        step(eng, "set_theta", lambda: eng.set_theta(theta))
        step(eng, "factorize", eng.factorize)
        step(eng, "predict M=200", lambda: eng.predict(Xs200))
        step(eng, "evaluate grad", lambda: eng.evaluate(theta, grad=True))
        step(eng, "predict M=200 (GEMM form)", lambda: eng.predict(Xs200))
        step(eng, "predict_grad", lambda: eng.predict_grad(Xs200))
        step(eng, "predict_with_grad", lambda: eng.predict_with_grad(Xs200))
        step(eng, "predict_joint M=150", lambda: eng.predict_joint(Xs150))
        step(eng, "draw_joint S=4", lambda: eng.draw_joint(Xs150, Z))
        step(eng, "append K=1", lambda: eng.append(X[300:301], y[300:301]))      # 300 -> 301: no re-layout
        step(eng, "append K=100", lambda: eng.append(X[301:401], y[301:401]))    # -> 401: Nr 384 -> 512, a re-layout
        step(eng, "truncate 250", lambda: eng.truncate(250))
        step(eng, "set_data N=130", lambda: eng.set_data(X[:130], y[:130]))
        step(eng, "set_theta (N=130)", lambda: eng.set_theta(theta))
        step(eng, "reserve grad M=200", lambda: eng.reserve(gradient=True, M=200))
        step(eng, "factorize (N=130)", eng.factorize)
        step(eng, "set_dist_mode 1", lambda: eng.set_dist_mode(1))
    # a kernel with another number of continuous dimensions behind set_data: the prepared points are laid out again
    spec2 = O.make_spec(D, range(2), kind="ExpQuad")
    theta2 = O.pack_theta(spec2, ls[:2], 1.0, 0.2)
    with Engine(0) as eng:
        step(eng, "second: set_data N=300", lambda: eng.set_data(X[:300], y[:300]))
        step(eng, "second: set_kernel n_cont=3", lambda: eng.set_kernel(kernel))
        step(eng, "second: set_theta", lambda: eng.set_theta(theta))
        step(eng, "second: set_kernel n_cont=2", lambda: eng.set_kernel(KernelSpec(D=D, idx_cont=[0, 1], kind="ExpQuad")))
        step(eng, "second: set_theta n_cont=2", lambda: eng.set_theta(theta2))
        step(eng, "second: factorize", eng.factorize)
    return out


@pytest.mark.gpu
def test_resident_ledger_matches_the_recorded_script(gpu):
    want = json.loads(GOLDEN.read_text())["steps"]
    got = ledger_script()
    for g, w in zip(got, want):
        print(f"LEDGER {g[0]:32s} resident {g[1]:>10d} peak {g[2]:>10d}   recorded {w[1]:>10d} {w[2]:>10d}")
    assert got == want


if __name__ == "__main__":
    Path(sys.argv[1]).write_text(json.dumps({"steps": ledger_script()}, indent=1) + "\n")
    print(Path(sys.argv[1]).read_text())
