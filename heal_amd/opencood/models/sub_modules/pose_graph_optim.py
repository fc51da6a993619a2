"""The 2-D agent-object pose graph of CoAlign on plain numpy (reference: opencood/models/sub_modules/pose_graph_optim.py, which
derives its PoseGraphOptimization2D from g2o.SparseOptimizer).  Same methods -- add_vertex, add_edge, optimize, get_pose -- and the
same cost; no g2o.  Host only, float64, imports nothing that touches a GPU.  heal_amd/csrc/pose_graph.hip solves the same problem
with the same steps on the device.

Cost.  SE(2) poses compose as a . b = (t_a + R_a t_b, th_a + th_b).  With x_i the pose vertex of an edge, x_j its landmark and z
the measurement,
    SE2 edge   e = vec(z^-1 . (x_i^-1 . x_j)) = (R_z^T (R_i^T (t_j - t_i) - t_z), wrap(th_j - th_i - th_z))
    XY edge    e = R_i^T (l_j - t_i) - z
and the objective is sum e^T Omega e over the edges (g2o's chi2; Omega is used through its diagonal, all the box alignment sets).
Angles are wrapped to (-pi, pi].

Solver.  Levenberg-Marquardt with g2o's damping rule (OptimizationAlgorithmLevenberg): lambda_0 = 1e-5 max diag(H); a trial
step solves (H + lambda I) d = b; rho = (chi - chi_trial) / (d . (lambda d + b) + 1e-3); on rho > 0 the step is kept and
lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2; otherwise lambda *= nu, nu *= 2.  Vertices are updated additively
(t += d_t, th = wrap(th + d_th)).  Every edge joins one pose vertex to one landmark, so the landmark blocks are eliminated in
closed form (3x3 inverses) and the dense system that is factored has 3 unknowns per free pose vertex.

Stopping rule (ours; g2o itself only stops on these or on max_iterations): an outer iteration ends the solve when ten consecutive
trial steps were rejected, when rho is exactly 0 (the trial cost equals the current one to the last bit), or when lambda is no
longer finite.  One more rule carries the solve past that point: a cost in float64 cannot tell two points apart whose costs differ by
less than ~1e-16 chi2, which is a distance of ~1e-8 from the minimiser, and the accept / reject test would stall there.  So a
trial step whose PREDICTED decrease d . (lambda d + b) is at most 1e-13 chi2 is taken without looking at its cost and without
touching lambda (by then lambda is far below diag(H): these are Gauss-Newton steps, which contract linearly on a problem with
non-zero residuals).  The solve ends after such a step when its largest component is at most 1e-14 (metres, radians) or more
than half the previous such step's (the rounding floor of the gradient).
g2o's own iterates are not reproduced; the target is the minimiser reached from the same start.
"""
import numpy as np

TAU = 1e-5          # lambda_0 = TAU * max diag(H)
MAX_TRIALS = 10     # consecutive rejected trial steps that end the solve
MAX_ITERATIONS = 1000
POLISH = 1e-13      # a trial step whose predicted decrease is <= POLISH * chi2 is taken without the cost test
STEP_FLOOR = 1e-14  # ... and the solve ends when such a step's largest component is below this (m, rad) or stops halving

STATUS_CONVERGED = 0        # stopped by the rule above
STATUS_MAX_ITERATIONS = 1
STATUS_NO_EDGES = 2         # nothing to optimise: every estimate is returned as it came
STATUS_ABANDONED = 3        # box alignment only: abandon_hard_cases returned the input
STATUS_NONFINITE = 4        # a non-finite input, cost or system: every estimate is returned as it came


def wrap_angle(theta):
    """theta -> (-pi, pi]"""
    return theta - 2.0 * np.pi * np.ceil((theta - np.pi) / (2.0 * np.pi))


class SE2:
    """What the box alignment uses of g2o.SE2: SE2(x, y, theta) or SE2([x, y, theta]); the angle is kept in (-pi, pi]."""

    def __init__(self, *args):
        v = np.asarray(args[0] if len(args) == 1 else args, dtype=np.float64).reshape(3)
        self._v = np.array([v[0], v[1], wrap_angle(v[2])])

    def vector(self):
        return self._v.copy()

    def translation(self):
        return self._v[:2].copy()

    def angle(self):
        return float(self._v[2])


def linearize(xi, xj, z, w):
    """Errors and Jacobians of E edges at once.  xi, xj [E,3] pose / landmark estimates, z [E,3] measurements, w [E,3] diagonal
    information; an XY edge is the row with z[2] = 0, w[2] = 0 (its third error is weighted out).  -> e [E,3], Ji, Jj [E,3,3]."""
    ci, si = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    cz, sz = np.cos(z[:, 2]), np.sin(z[:, 2])
    dx, dy = xj[:, 0] - xi[:, 0], xj[:, 1] - xi[:, 1]
    d0, d1 = ci * dx + si * dy, -si * dx + ci * dy
    u0, u1 = d0 - z[:, 0], d1 - z[:, 1]
    e = np.stack([cz * u0 + sz * u1, -sz * u0 + cz * u1, wrap_angle(xj[:, 2] - xi[:, 2] - z[:, 2])], axis=1)
    e[:, 2] = np.where(w[:, 2] != 0.0, e[:, 2], 0.0)
    zero, one = np.zeros_like(ci), np.ones_like(ci)
    Z = np.stack([cz, sz, zero, -sz, cz, zero, zero, zero, one], axis=1).reshape(-1, 3, 3)
    Ji = Z @ np.stack([-ci, -si, d1, si, -ci, -d0, zero, zero, -one], axis=1).reshape(-1, 3, 3)
    Jj = Z @ np.stack([ci, si, zero, -si, ci, zero, zero, zero, one], axis=1).reshape(-1, 3, 3)
    return e, Ji, Jj


class PoseGraphOptimization2D:
    def __init__(self, verbose=False):
        self.verbose = verbose
        self._vertices = {}            # id -> dict(estimate float64 [3] or [2], fixed, se2), in insertion order
        self._edges = []               # dict(vertices (i, j), measurement [3] or [2], information [d,d], se2)
        self.iterations = 0
        self.status = STATUS_NO_EDGES
        self.chi2_initial = 0.0
        self.chi2_final = 0.0

    # ---- the reference's surface -----------------------------------------------------------------------------------------
    def add_vertex(self, id, pose, fixed=False, SE2=True):
        est = pose.vector() if hasattr(pose, "vector") else np.asarray(pose, dtype=np.float64).reshape(-1).copy()
        if SE2:
            est = globals()["SE2"](est).vector()
        self._vertices[int(id)] = {"estimate": est, "fixed": bool(fixed), "se2": bool(SE2)}

    def add_edge(self, vertices, measurement, information=np.identity(3), robust_kernel=None, SE2=True):
        if robust_kernel is not None:
            raise NotImplementedError("robust kernels are not part of the box alignment")
        z = measurement.vector() if hasattr(measurement, "vector") else np.asarray(measurement, dtype=np.float64).reshape(-1).copy()
        self._edges.append({"vertices": (int(vertices[0]), int(vertices[1])), "measurement": z,
                            "information": np.array(information, dtype=np.float64), "se2": bool(SE2)})

    def get_pose(self, id):
        v = self._vertices[int(id)]
        return SE2(v["estimate"]) if v["se2"] else v["estimate"].copy()

    def vertex_list(self):
        return [(i, v["fixed"], v["se2"], v["estimate"].copy()) for i, v in self._vertices.items()]

    def edge_list(self):
        return [(e["vertices"], e["se2"], e["measurement"].copy(), e["information"].copy()) for e in self._edges]

    # ---- arrays ----------------------------------------------------------------------------------------------------------
    def _pack(self):
        poses = sorted({e["vertices"][0] for e in self._edges})
        marks = sorted({e["vertices"][1] for e in self._edges})
        if set(poses) & set(marks):
            raise ValueError("every edge must join a pose vertex (first) to a landmark vertex (second)")
        for i in poses:
            if not self._vertices[i]["se2"]:
                raise ValueError(f"vertex {i} is the first vertex of an edge and must be SE2")
        pi = {v: k for k, v in enumerate(poses)}
        mi = {v: k for k, v in enumerate(marks)}
        E = len(self._edges)
        ia = np.array([pi[e["vertices"][0]] for e in self._edges], dtype=np.int64)
        jl = np.array([mi[e["vertices"][1]] for e in self._edges], dtype=np.int64)
        z, w = np.zeros((E, 3)), np.zeros((E, 3))
        for k, e in enumerate(self._edges):
            d = 3 if e["se2"] else 2
            if self._vertices[e["vertices"][1]]["se2"] != e["se2"]:
                raise ValueError("an SE2 edge needs an SE2 landmark and an XY edge an XY landmark")
            z[k, :d] = e["measurement"][:d]
            w[k, :d] = np.diag(e["information"])[:d]
        Xp = np.array([self._vertices[v]["estimate"] for v in poses], dtype=np.float64).reshape(-1, 3)
        Xl = np.zeros((len(marks), 3))
        for k, v in enumerate(marks):
            est = self._vertices[v]["estimate"]
            Xl[k, :len(est)] = est
        free_p = np.array([not self._vertices[v]["fixed"] for v in poses], dtype=bool)
        free_l = np.array([not self._vertices[v]["fixed"] for v in marks], dtype=bool)
        se2_l = np.array([self._vertices[v]["se2"] for v in marks], dtype=bool)
        return poses, marks, ia, jl, z, w, Xp, Xl, free_p, free_l, se2_l

    @staticmethod
    def _chi2(Xp, Xl, ia, jl, z, w):
        e, _, _ = linearize(Xp[ia], Xl[jl], z, w)
        return float(np.sum(w * e * e))

    def chi2(self):
        if not self._edges:
            return 0.0
        _, _, ia, jl, z, w, Xp, Xl, _, _, _ = self._pack()
        return self._chi2(Xp, Xl, ia, jl, z, w)

    def gradient(self):
        """d chi2 / d (every free vertex's coordinates), additive parametrisation: {vertex id: [3] or [2]}."""
        out = {}
        if not self._edges:
            return out
        poses, marks, ia, jl, z, w, Xp, Xl, free_p, free_l, se2_l = self._pack()
        e, Ji, Jj = linearize(Xp[ia], Xl[jl], z, w)
        we = (w * e)[:, :, None]
        gp, gl = np.zeros_like(Xp), np.zeros_like(Xl)
        np.add.at(gp, ia, 2.0 * np.sum(Ji * we, axis=1))
        np.add.at(gl, jl, 2.0 * np.sum(Jj * we, axis=1))
        for k, v in enumerate(poses):
            if free_p[k]:
                out[v] = gp[k]
        for k, v in enumerate(marks):
            if free_l[k]:
                out[v] = gl[k, :3 if se2_l[k] else 2]
        return out

    # ---- the solve -------------------------------------------------------------------------------------------------------
    def optimize(self, max_iterations=MAX_ITERATIONS):
        max_iterations = int(min(max(max_iterations, 0), MAX_ITERATIONS))
        self.iterations, self.status = 0, STATUS_NO_EDGES
        self.chi2_initial = self.chi2_final = 0.0
        if not self._edges:
            return 0
        poses, marks, ia, jl, z, w, Xp, Xl, free_p, free_l, se2_l = self._pack()
        P, L = len(poses), len(marks)
        chi = self._chi2(Xp, Xl, ia, jl, z, w)
        self.chi2_initial = self.chi2_final = chi
        if not np.isfinite(chi):
            self.status = STATUS_NONFINITE
            return 0
        dimmask_l = np.where(se2_l[:, None], 1.0, np.array([1.0, 1.0, 0.0])[None, :]) * free_l[:, None]   # [L,3] live coordinates
        dimmask_p = np.repeat(free_p[:, None], 3, axis=1).astype(np.float64)
        lam, nu, polished, step, last_step = 0.0, 2.0, False, 0.0, None
        self.status = STATUS_MAX_ITERATIONS
        eye3 = np.eye(3)
        for it in range(max_iterations):
            e, Ji, Jj = linearize(Xp[ia], Xl[jl], z, w)
            chi = float(np.sum(w * e * e))
            JiW = Ji * w[:, :, None]                                   # Omega Ji
            JjW = Jj * w[:, :, None]
            Hpp, Hll, Wpl = np.zeros((P, 3, 3)), np.zeros((L, 3, 3)), np.zeros((L, P, 3, 3))
            bp, bl = np.zeros((P, 3)), np.zeros((L, 3))
            np.add.at(Hpp, ia, np.einsum("erp,erq->epq", JiW, Ji))
            np.add.at(Hll, jl, np.einsum("erp,erq->epq", JjW, Jj))
            np.add.at(Wpl, (jl, ia), np.einsum("erp,erq->epq", JiW, Jj))
            np.add.at(bp, ia, -np.einsum("erp,er->ep", JiW, e))
            np.add.at(bl, jl, -np.einsum("erp,er->ep", JjW, e))
            # fixed vertices and the missing yaw of an XY landmark leave the system: zero rows and columns, unit diagonal
            Hpp *= dimmask_p[:, :, None] * dimmask_p[:, None, :]
            Hll *= dimmask_l[:, :, None] * dimmask_l[:, None, :]
            Wpl *= dimmask_p[None, :, :, None] * dimmask_l[:, None, None, :]
            bp *= dimmask_p
            bl *= dimmask_l
            if it == 0:
                diag = np.concatenate([np.einsum("pii->pi", Hpp).ravel(), np.einsum("lii->li", Hll).ravel()])
                lam = TAU * float(diag.max())
            self.iterations = it + 1
            rho, trials = 0.0, 0
            while True:
                ok = True
                Ml = Hll + lam * eye3[None]
                Ml += (1.0 - dimmask_l)[:, :, None] * eye3[None]          # dead coordinates: 1 on the diagonal
                try:
                    Minv = np.linalg.inv(Ml)
                    yl = np.einsum("lpq,lq->lp", Minv, bl)
                    WM = np.einsum("lapq,lqr->lapr", Wpl, Minv)              # W Minv
                    S = -np.einsum("lapr,lbqr->apbq", WM, Wpl)
                    for a in range(P):
                        S[a, :, a, :] += Hpp[a] + lam * eye3 + np.diag(1.0 - dimmask_p[a])
                    r = bp - np.einsum("lapq,lq->ap", Wpl, yl)
                    S2, r2 = S.reshape(3 * P, 3 * P), r.reshape(3 * P)
                    c = np.linalg.cholesky(S2)
                    dp = np.linalg.solve(c.T, np.linalg.solve(c, r2)).reshape(P, 3)
                    dl = yl - np.einsum("lapq,ap->lq", WM, dp)
                    ok = bool(np.all(np.isfinite(dp)) and np.all(np.isfinite(dl)))
                except np.linalg.LinAlgError:
                    ok = False
                if ok:
                    Xp_t, Xl_t = Xp + dp, Xl + dl
                    Xp_t[:, 2] = wrap_angle(Xp_t[:, 2])
                    Xl_t[:, 2] = np.where(se2_l, wrap_angle(Xl_t[:, 2]), 0.0)
                    chi_t = self._chi2(Xp_t, Xl_t, ia, jl, z, w)
                    pred = float(np.sum(dp * (lam * dp + bp)) + np.sum(dl * (lam * dl + bl)))
                    if pred <= POLISH * chi:                         # below the cost's resolution: taken unseen (see above)
                        step = float(max(np.abs(dp).max(initial=0.0), np.abs(dl).max(initial=0.0)))
                        Xp, Xl, chi, polished = Xp_t, Xl_t, min(chi, chi_t), True
                        break
                    rho = (chi - chi_t) / (pred + 1e-3)
                else:
                    chi_t, rho = np.inf, -1.0
                if ok and rho > 0.0 and np.isfinite(chi_t):
                    alpha = min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    nu = 2.0
                    Xp, Xl, chi = Xp_t, Xl_t, chi_t
                else:
                    lam *= nu
                    nu *= 2.0
                trials += 1
                if not (rho < 0.0 and trials < MAX_TRIALS and np.isfinite(lam)):
                    break
            self.chi2_final = chi
            if polished:
                if step <= STEP_FLOOR or (last_step is not None and step > 0.5 * last_step):
                    self.status = STATUS_CONVERGED
                    break
                last_step, polished = step, False
                continue
            last_step = None
            if self.verbose:
                print(f"iteration {it}: chi2 {chi:.12g} lambda {lam:.6g} trials {trials}")
            if trials == MAX_TRIALS or rho == 0.0 or not np.isfinite(lam):
                self.status = STATUS_CONVERGED
                break
        for k, v in enumerate(poses):
            if free_p[k]:
                self._vertices[v]["estimate"] = Xp[k].copy()
        for k, v in enumerate(marks):
            if free_l[k]:
                self._vertices[v]["estimate"] = Xl[k, :3 if se2_l[k] else 2].copy()
        return self.iterations
