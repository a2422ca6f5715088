"""The Cauchy-robust between factor as include/rolo_hip.h states it, in numpy on top of tests/pgo_twin.py: the statement the device code is held to.

A between factor may carry a loss constant k > 0. With e_w = e / sigma and r^2 = |e_w|^2 its cost term is rho = k^2 / 2 log1p(r^2 / k^2) in place of r^2 / 2
(mEstimator::Cauchy::loss) and its weight w = k^2 / (k^2 + r^2) (::weight); the whitened error and both whitened Jacobians are scaled by sqrt(w) before the
products (noiseModel::Robust::WhitenSystem), so the factor's blocks are w J^T J and its gradient parts w J^T e_w, the exact gradient of rho. Everything else,
the step and the outer loop, is pgo_twin.Graph's: accept, reject and convergence read the robust cost."""
import numpy as np

import pgo_twin as tw


class Graph(tw.Graph):
    def __init__(self):
        super().__init__()
        self.k = []          # per factor: None (no loss) or the Cauchy constant

    def add_prior(self, i, T, var6):
        super().add_prior(i, T, var6); self.k.append(None)

    def add_between(self, i, j, T, var6, k=None):
        assert k is None or (np.isfinite(k) and k > 0)
        super().add_between(i, j, T, var6); self.k.append(None if k is None else float(k))

    def whitened(self, f, poses=None):
        """e_w and the whitened Jacobians before any loss"""
        return super().factor(f, poses)

    def r2_weight_rho(self, f, poses=None):
        e = self.whitened(f, poses)[0]
        r2 = e @ e
        if self.k[f] is None:
            return r2, 1.0, 0.5 * r2
        k2 = self.k[f] * self.k[f]
        return r2, k2 / (k2 + r2), 0.5 * k2 * np.log1p(r2 / k2)

    def factor(self, f, poses=None):
        """sqrt(w) e_w, sqrt(w) J_i, sqrt(w) J_j: the system as Robust::WhitenSystem leaves it"""
        e, Ji, Jj = self.whitened(f, poses)
        if self.k[f] is None:
            return e, Ji, Jj
        k2 = self.k[f] * self.k[f]
        s = np.sqrt(k2 / (k2 + e @ e))
        return s * e, s * Ji, None if Jj is None else s * Jj

    def cost(self, poses=None):
        c = 0.0
        for f in range(len(self.factors)):
            c += self.r2_weight_rho(f, poses)[2]
        return c

    def linearize(self):
        """as pgo_twin.Graph.linearize; the cost is the sum of rho, the gradient and the blocks are those of the reweighted system"""
        N = len(self.poses)
        g = np.zeros((N, 6)); Dg = np.zeros((N, 6, 6)); Ch = np.zeros((max(N - 1, 0), 6, 6)); chord = []; chord_ij = []
        cost = 0.0
        for f, (i, j, _, _) in enumerate(self.factors):
            e, Ji, Jj = self.factor(f)
            cost += self.r2_weight_rho(f)[2]
            g[i] += Ji.T @ e; Dg[i] += Ji.T @ Ji
            if j >= 0:
                g[j] += Jj.T @ e; Dg[j] += Jj.T @ Jj
                Hij = Ji.T @ Jj
                if j == i + 1: Ch[i] += Hij
                elif i == j + 1: Ch[j] += Hij.T
                else: chord.append(Hij); chord_ij.append((i, j))
        return cost, g.reshape(-1), Dg, Ch, np.array(chord).reshape(-1, 6, 6), np.array(chord_ij, np.int32).reshape(-1, 2)

    def factor_errors(self, poses=None):
        """-> r^2 and w of every factor at the poses; w is exactly 1.0 for a factor without loss"""
        rw = [self.r2_weight_rho(f, poses)[:2] for f in range(len(self.factors))]
        return np.array([x[0] for x in rw], np.float64), np.array([x[1] for x in rw], np.float64)


def build(spec, graph=None, plain=False):
    """pgo_twin.build for a spec that may hold `loss`: one entry per between, None or k. plain: every loss dropped"""
    g = Graph() if graph is None else graph
    loss = spec.get("loss", [None] * len(spec["betweens"]))
    assert len(loss) == len(spec["betweens"])
    for X in spec["initial"]:
        g.add_pose(tw.T_of(X))
    for i, T, v in spec["priors"]:
        g.add_prior(i, T, v)
    for (i, j, T, v), k in zip(spec["betweens"], loss):
        g.add_between(i, j, T, v, None if plain else k)
    return g


# ---- the test graphs of pgo_twin with their extra factors robust ----
ROBUST_KINDS = ("one", "reversed", "skip2", "pair2", "chain2")


def robust_case_spec(N, kind, perturb=(1e-2, 5e-2), k=1.0):
    """pgo_twin.case_spec with the factors `kind` adds under a Cauchy loss; of pair2's two factors the first is robust and the second plain"""
    assert kind in ROBUST_KINDS
    spec = tw.case_spec(N, kind, perturb=perturb)
    extra = len(spec["betweens"]) - (N - 1)
    spec["loss"] = [None] * (N - 1) + ([k, None] if kind == "pair2" else [k] * extra)
    return spec


# ---- outlier graphs: a circuit with its true loops and two false "same place" loops a quarter lap apart ----
OUTLIER_SIZES = (65, 120)


def false_loops(N):
    return [(N - 1, N - 1 - N // 4), (N - 4, N - 9 - N // 4)]


def outlier_spec(N, k=1.0, outliers=True):
    """circuit(N, 4, seed=N); with outliers two false loops with Z = I and variances 0.3 after the true ones; every loop under Cauchy(k), chain and prior plain.
    spec["true_loops"] / ["false_loops"]: their factor indices in a graph built from the spec (the prior is factor 0)"""
    spec = tw.circuit(N, 4, seed=N)
    n_true = len(spec["betweens"]) - (N - 1)
    fl = false_loops(N) if outliers else []
    for i, j in fl:
        spec["betweens"].append((i, j, np.eye(4), np.full(6, 0.3)))
    spec["loss"] = [None] * (N - 1) + [k] * (n_true + len(fl))
    first = len(spec["priors"]) + N - 1
    spec["true_loops"] = list(range(first, first + n_true))
    spec["false_loops"] = list(range(first + n_true, first + n_true + len(fl)))
    return spec


# ---- a graph grown as the back end grows it: one key pose per step, events arriving while it grows ----
LIFE_POSES = 200


def life_script(N=LIFE_POSES, seed=9):
    """-> (steps, spec). steps: one list of operations per call of optimize, ("pose", k, Z) (key pose k, its odometry measurement Z from k - 1; for k = 0 its
    prior follows), ("prior", i, T, var6), ("between", i, j, T, var6, k or None); steps named in `events` carry more than the key pose. spec: the whole graph
    in the form of pgo_twin.circuit plus `loss`, its `factors` in the order the steps add them, starting from the composed odometry. Measurements are truth
    plus 1 mrad / 1 cm. The events: a loop from the newest pose to an old one; two loops in one step; a loop between two old poses in a step without a pose;
    a loop under Cauchy(1); a second factor on an old consecutive pair (it lands in that pose's chain block, reversed); a prior on an old pose; a loop to pose 0;
    and a second factor on the newest pair (N - 2, N - 1) in a step without a pose"""
    c = tw.circuit(N, 0, seed=seed)
    rng = np.random.default_rng(900 + seed)
    tr = c["truth"]
    noise = lambda: np.concatenate([rng.normal(0, 1e-3, 3), rng.normal(0, 1e-2, 3)])
    meas = lambda i, j: tw.T_of(tw.mul(tw.mul(tw.inv(*tr[i]), tr[j]), tw.exp_se3(noise())))
    lv, ov = np.full(6, 1e-2), np.array(tw.ODOM_VARIANCES)
    loop = lambda i, j, k=None: ("between", i, j, meas(i, j), lv, k)
    at = {40: [loop(40, 5)], 60: [loop(60, 20), loop(60, 33)], 90: [loop(90, 30, 1.0)], 110: [("between", 71, 70, meas(71, 70), ov, None)],
          130: [("prior", 100, tw.T_of(tr[100]), np.full(6, 1e-2))], 150: [loop(150, 0)]}
    alone = {75: [loop(50, 10)], 170: [("between", 170, 169, meas(170, 169), ov, None)]}      # after key pose 75 (170): a step that adds no pose
    steps, events = [], []
    for k in range(N):
        ops = [("pose", k, None if k == 0 else c["betweens"][k - 1][2])]
        if k == 0:
            ops.append(("prior", 0, c["priors"][0][1], c["priors"][0][2]))
        if k in at:
            ops += at[k]; events.append(len(steps))
        steps.append(ops)
        if k in alone:
            events.append(len(steps)); steps.append(list(alone[k]))
    factors = []
    for ops in steps:
        for op in ops:
            if op[0] == "pose" and op[1] > 0: factors.append(("between", op[1] - 1, op[1], op[2], ov, None))
            elif op[0] != "pose": factors.append(op)
    return steps, dict(truth=tr, initial=c["initial"], factors=factors, events=events)


def build_life(spec):
    """the twin's graph of life_script's whole graph, the factors in the order the steps added them"""
    g = Graph()
    for X in spec["initial"]:
        g.add_pose(tw.T_of(X))
    for f in spec["factors"]:
        if f[0] == "prior": g.add_prior(f[1], f[2], f[3])
        else: g.add_between(f[1], f[2], f[3], f[4], f[5])
    return g


def grow_life(steps, first_pose, add_pose, add_prior, add_between, last_pose, after_step):
    """drives a graph through life_script's steps: a new key pose starts at the graph's last pose times its odometry measurement, as the back end's does"""
    for n, ops in enumerate(steps):
        for op in ops:
            if op[0] == "pose":
                if op[1] == 0:
                    add_pose(first_pose)
                else:
                    add_pose(last_pose() @ op[2]); add_between(op[1] - 1, op[1], op[2], np.array(tw.ODOM_VARIANCES), None)
            elif op[0] == "prior": add_prior(*op[1:])
            else: add_between(*op[1:])
        after_step(n, ops)
