"""One Problem.solve with a user cost plug-in (the host objective, opty/direct_collocation.py) on exp_14: a wrapped CostAirVel(12)
(a known cost in disguise) and CostAirVel + phi^4 + v-smoothness (no class expresses it).  Prints wall time (best of 3 after a
warm-up), outer iterations, Newton steps per subproblem and the cost / cost_grad call counts."""
import contextlib
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tests')]
import d2d.opty_utils as d2ou                      # noqa: E402
import d2d.optyplan_scenarios as sc                # noqa: E402
import single_opt_planner as sop                   # noqa: E402
from test_gpu_user_cost import Smooth, Wrapped     # noqa: E402


class wrapped(sc.exp_14):
    cost = Wrapped(d2ou.CostAirVel(12))


class smooth(sc.exp_14):
    cost = Smooth()


for s in (wrapped, smooth, sc.exp_14):
    with contextlib.redirect_stdout(io.StringIO()):
        p = sop.Planner(s, backend='nlp')
    x0 = p.get_initial_guess('tri')
    ts = []
    for _ in range(4):
        t0 = time.perf_counter()
        sol, info = p.prob.solve(x0)
        ts.append(time.perf_counter() - t0)
    print(f"{s.__name__:8s} {p.prob.objective:7s} Problem.solve {1e3 * min(ts[1:]):7.1f} ms (first {1e3 * ts[0]:.1f})  status {info['status_msg']}"
          f"  cost {info['obj_val']:.9f}  outer {info.get('outer', '-')}  Newton steps per subproblem {info.get('sub_iters', info['iters'])}"
          f"  cost calls {info.get('cost_calls', '-')}  cost_grad calls {info.get('grad_calls', '-')}")
