"""Host-side mirror of g2o's non-linear drivers over the device-resident solver.

`levenberg_solve_iteration` restates OptimizationAlgorithmLevenberg::solve
(/root/reference/g2o/core/optimization_algorithm_levenberg.cpp:57-146) and
`gauss_newton_iteration` OptimizationAlgorithmGaussNewton::solve
(/root/reference/g2o/core/optimization_algorithm_gauss_newton.cpp:50-93), written against a small
"graph" protocol so the same loop drives the GPU solver (estimates, errors and Jacobians stay in
HBM) and, in the tests, the CPU oracle:

    graph.compute_active_errors()   SparseOptimizer::computeActiveErrors   sparse_optimizer.cpp:61-76
    graph.linearize()               errors + Jacobians (what buildSystem's per-edge linearizeOplus needs)
    graph.chi2()                    activeRobustChi2                        sparse_optimizer.cpp:100-114
    graph.update()                  update(solver.x())                      sparse_optimizer.cpp:421-434
    graph.push() / pop() / discard_top()                                    sparse_optimizer.cpp:599-650
    solver.buildSystem/setLambda/solve/restoreDiagonal/maxDiagonal/computeScale   (Solver interface)
"""
import math

OK, TERMINATE, FAIL = 1, 0, -1          # OptimizationAlgorithm::SolverResult (optimization_algorithm.h:49)
DBL_MAX = 1.7976931348623157e308


class LevenbergState:
    """The members of OptimizationAlgorithmLevenberg (optimization_algorithm_levenberg.h:83-96)."""

    def __init__(self, tau=1e-5, max_trials=10, user_lambda_init=0.0):
        self.tau = tau
        self.good_step_upper = 2.0 / 3.0
        self.good_step_lower = 1.0 / 3.0
        self.max_trials = max_trials
        self.user_lambda_init = user_lambda_init
        self.current_lambda = -1.0
        self.ni = 2.0
        self.levenberg_iterations = 0


def levenberg_solve_iteration(graph, solver, st, iteration):
    graph.linearize()                                   # computeActiveErrors + per-edge linearizeOplus
    current_chi = graph.chi2()
    temp_chi = current_chi
    solver.buildSystem()
    if iteration == 0:                                  # computeLambdaInit :149-163
        st.current_lambda = st.user_lambda_init if st.user_lambda_init > 0 else st.tau * solver.maxDiagonal()
        st.ni = 2.0
    rho = 0.0
    qmax = 0
    # device-resident graph + HIP solver: the trial's three host round trips (solve status, chi2, computeScale) collapse
    # into one (g2ohip_solve_async / g2ohip_trial_stats); same values, same decisions
    fused = getattr(graph, "device_resident", False) and hasattr(solver, "solveAsync") and hasattr(solver, "trialStats")
    while True:
        graph.push()
        solver.setLambda(st.current_lambda, True)
        if fused:
            solver.solveAsync()
            graph.update()
            solver.restoreDiagonal()
            graph.compute_active_errors()
            ok2, temp_chi, sc = solver.trialStats(st.current_lambda)
            if ok2 is None:      # the asynchronous solve has to be repeated (g2ohip_trial_stats status 2): redo the trial in
                graph.pop()      # the synchronous form, which retries by itself -- same values, same decisions
                graph.push()
                solver.setLambda(st.current_lambda, True)
                ok2 = solver.solve()
                graph.update()
                solver.restoreDiagonal()
                graph.compute_active_errors()
                temp_chi = graph.chi2()
                sc = solver.computeScale(st.current_lambda) if ok2 else 0.0
        else:
            ok2 = solver.solve()
            graph.update()
            solver.restoreDiagonal()
            graph.compute_active_errors()
            temp_chi = graph.chi2()
            sc = solver.computeScale(st.current_lambda) if ok2 else 0.0
        if not ok2:
            temp_chi = DBL_MAX
        rho = current_chi - temp_chi
        scale = (sc if ok2 else 0.0) + 1e-3             # computeScale :165-172
        rho /= scale
        if rho > 0 and math.isfinite(temp_chi):         # last step was good
            alpha = 1.0 - (2.0 * rho - 1.0) ** 3
            alpha = min(alpha, st.good_step_upper)
            st.current_lambda *= max(st.good_step_lower, alpha)
            st.ni = 2.0
            current_chi = temp_chi
            graph.discard_top()
        else:
            st.current_lambda *= st.ni
            st.ni *= 2.0
            graph.pop()
        qmax += 1
        if not (rho < 0 and qmax < st.max_trials):
            break
    st.levenberg_iterations = qmax
    result = TERMINATE if (qmax == st.max_trials or rho == 0) else OK
    return result, current_chi


def gauss_newton_iteration(graph, solver):
    graph.linearize()
    chi = graph.chi2()
    solver.buildSystem()
    if not solver.solve():
        return FAIL, chi
    graph.update()
    return OK, chi


class DoglegState:
    """The members of OptimizationAlgorithmDogleg (optimization_algorithm_dogleg.cpp:40-50, .h:83-100)."""

    def __init__(self, initial_delta=1e4, max_trials_after_failure=100, initial_lambda=1e-7, lambda_factor=10.0):
        self.delta = initial_delta
        self.max_trials = max_trials_after_failure
        self.current_lambda = initial_lambda
        self.lambda_factor = lambda_factor
        self.was_pd = True
        self.last_step = "Undefined"
        self.last_num_tries = 0


def dogleg_solve_iteration(graph, solver, st):
    """OptimizationAlgorithmDogleg::solve (optimization_algorithm_dogleg.cpp:57-207).  Needs solver.b(), x(), setX(),
    multiplyHessian(v) (dest += H v from a zero dest, block_solver.h:142) besides the LM protocol."""
    import numpy as np
    graph.linearize()                                   # computeActiveErrors + the Jacobians buildSystem needs
    current_chi = graph.chi2()
    solver.buildSystem()
    b = solver.b()
    aux = solver.multiplyHessian(b)
    alpha = float(b @ b) / float(aux @ b)
    hsd = alpha * b
    hsd_norm = float(np.linalg.norm(hsd))
    hgn = None
    hgn_norm = -1.0
    good = False
    tries = 0
    while True:
        tries += 1
        if hgn is None:
            min_lambda, max_lambda = 1e-12, 1e3
            ok = False
            while not ok:                               # damp only once the matrix was seen not positive definite
                if not st.was_pd:
                    solver.setLambda(st.current_lambda, True)
                ok = solver.solve()
                if not st.was_pd:
                    solver.restoreDiagonal()
                st.was_pd = st.was_pd and ok
                if not st.was_pd:
                    if ok:
                        st.current_lambda = max(min_lambda, st.current_lambda / (0.5 * st.lambda_factor))
                    else:
                        st.current_lambda *= st.lambda_factor
                        if st.current_lambda > max_lambda:
                            st.current_lambda = max_lambda
                            return FAIL, current_chi
            hgn = solver.x()
            hgn_norm = float(np.linalg.norm(hgn))
        if hgn_norm < st.delta:
            hdl = hgn
            st.last_step = "GN"
        elif hsd_norm > st.delta:
            hdl = st.delta / hsd_norm * hsd
            st.last_step = "Descent"
        else:
            d = hgn - hsd
            c = float(hsd @ d)
            bma = float(d @ d)
            if c <= 0.0:
                beta = (-c + math.sqrt(c * c + bma * (st.delta * st.delta - float(hsd @ hsd)))) / bma
            else:
                hs2 = float(hsd @ hsd)
                beta = (st.delta * st.delta - hs2) / (c + math.sqrt(c * c + bma * (st.delta * st.delta - hs2)))
            hdl = hsd + beta * d
            st.last_step = "Dogleg"
        aux = solver.multiplyHessian(hdl)
        linear_gain = -1.0 * float(aux @ hdl) + 2.0 * float(b @ hdl)
        graph.push()
        solver.setX(hdl)
        graph.update()
        graph.compute_active_errors()
        new_chi = graph.chi2()
        nonlinear_gain = current_chi - new_chi
        if abs(linear_gain) < 1e-12:
            linear_gain = 1e-12
        rho = nonlinear_gain / linear_gain
        if rho > 0:
            graph.discard_top()
            good = True
        else:
            graph.pop()
        if rho > 0.75:
            st.delta = max(st.delta, 3.0 * float(np.linalg.norm(hdl)))
        elif rho < 0.25:
            st.delta *= 0.5
        if good or tries >= st.max_trials:
            break
    st.last_num_tries = tries
    if tries == st.max_trials or not good:
        return TERMINATE, current_chi
    return OK, current_chi


BATCH_STAT_FIELDS = ("iteration", "numVertices", "numEdges", "chi2", "timeResiduals", "timeLinearize", "timeQuadraticForm",
                     "timeSchurComplement", "timeSymbolicDecomposition", "timeNumericDecomposition", "timeLinearSolution",
                     "iterationsLinearSolver", "timeUpdate", "timeIteration", "levenbergIterations", "timeLinearSolver",
                     "hessianDimension", "hessianPoseDimension", "hessianLandmarkDimension", "choleskyNNZ", "timeMarginals")


def format_batch_stats(st):
    """One line per iteration in the format of `g2o -stats <file>`: operator<<(ostream&, const G2OBatchStatistics&),
    /root/reference/g2o/core/batch_stats.cpp:49-82 (PTHING(s) = "s= value\t ", same field order)."""
    def fmt(v):
        return "%d" % v if isinstance(v, int) else "%g" % v
    return "".join("%s= %s\t " % (k, fmt(st.get(k, 0))) for k in BATCH_STAT_FIELDS)


def optimize(graph, solver, iterations, algorithm="lm", stats=None, num_vertices=0, num_edges=0, times=None, **lm_args):
    """SparseOptimizer::optimize (sparse_optimizer.cpp:354-419): returns (#iterations done, chi2 per
    iteration before its step, lambda per iteration, LM trials per iteration).
    stats: a list that receives one G2OBatchStatistics-like dict per iteration (sparse_optimizer.cpp:379-399; the solver
    must have profiling on for the per-stage times): write them with format_batch_stats for a `-stats` compatible file.
    times: a list that receives the wall-clock seconds of every iteration (each ends with a read-back, so they are exact)."""
    import time
    st = DoglegState(**lm_args) if algorithm == "dogleg" else LevenbergState(**lm_args)
    chis, lams, trials = [], [], []
    done = 0
    for it in range(iterations):
        ts = time.perf_counter()
        if algorithm == "dogleg":
            res, _ = dogleg_solve_iteration(graph, solver, st)
            lams.append(st.delta)
            trials.append(st.last_num_tries)
        elif algorithm == "lm":
            res, _ = levenberg_solve_iteration(graph, solver, st, it)
            lams.append(st.current_lambda)
            trials.append(st.levenberg_iterations)
        else:
            res, _ = gauss_newton_iteration(graph, solver)
        graph.compute_active_errors()
        chis.append(graph.chi2())
        done += 1
        if times is not None:
            times.append(time.perf_counter() - ts)
        if stats is not None:
            d = dict(solver.stats()) if hasattr(solver, "stats") else {}
            d.update(iteration=it, numVertices=int(num_vertices), numEdges=int(num_edges), chi2=chis[-1],
                     timeIteration=time.perf_counter() - ts, levenbergIterations=int(trials[-1]) if algorithm == "lm" else 0)
            for k in ("hessianDimension", "hessianPoseDimension", "hessianLandmarkDimension", "choleskyNNZ", "iterationsLinearSolver"):
                d[k] = int(d.get(k, 0))
            stats.append(d)
        if res != OK:
            break
    return done, chis, lams, trials


class DeviceBAGraph:
    """The graph protocol over HipBlockSolver's device-resident BA front end."""

    device_resident = True

    def __init__(self, solver):
        self.s = solver

    def linearize(self):
        self.s.baLinearize(True)

    def compute_active_errors(self):
        self.s.baLinearize(False)

    def chi2(self):
        return self.s.chi2()

    def update(self):
        self.s.baUpdate()

    def push(self):
        self.s.baPush()

    def pop(self):
        self.s.baPop()

    def discard_top(self):
        self.s.baDiscardTop()


def setup_device_ba(prob, huber_delta=0.0, device=0, options=None, huber_delta_pose=0.0):
    """Build a HipBlockSolver for an openslam_g2o_amd.synthetic BA problem with the estimates, errors
    and Jacobians produced on the device.  Returns (solver, graph).  options: g2ohip_set_option pairs that have to be
    in place before buildStructure (ordering / kernel selection knobs).  A problem with observation = "stereo"
    (make_ba_problem(..., stereo_baseline=b)) is a set of EdgeProjectXYZ2UVU: error_dim 3, bound through baSetStereoEdges.
    A problem with pose_edges (synthetic.make_ba_odometry, g2o_io.read_g2o_ba of a file with EDGE_SE3:EXPMAP) gets a second,
    binary set of EdgeSE3Expmap constraints between its cameras, bound through baSetPoseEdges; huber_delta_pose > 0 puts a Huber
    kernel on that set.  Its id is the projection set's + 1.
    A problem with observation = "inverse_depth" (synthetic.make_ba_inverse_depth) is a set of three-vertex EdgeProjectPSI2UV
    observations: the three binary sets of prob["pairs"] with their parts (ids 0, 1, 2 = solver.psi_sets), bound through
    baSetInverseDepthEdges with the information matrices prob["info"] [E][4] if present; huber_delta goes to all three of them.
    A pose set follows with id 3."""
    import numpy as np
    from . import capi
    stereo = prob.get("observation") == "stereo"
    psi = prob.get("observation") == "inverse_depth"
    s = capi.HipBlockSolver(6, 3, device)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    if psi:
        parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
        s.psi_sets = []
        for (v0, v1), pt in zip(prob["pairs"], parts):
            s.psi_sets.append(s.addEdgeSet(2, v0, v1))
            s.setEdgeSetParts(s.psi_sets[-1], pt)
        k = s.psi_sets[0]
    else:
        k = s.addEdgeSet(3 if stereo else 2, prob["v0"], prob["v1"])
    pe = prob.get("pose_edges")
    if pe is not None:
        kp = s.addEdgeSet(6, pe["v0"], pe["v1"])
    s.buildStructure(prob["nP"], prob["nL"], True)
    if psi:
        s.baSetInverseDepthEdges(*s.psi_sets, prob["cam_idx"], prob["anchor_idx"], prob["pt_idx"], prob["meas"], prob.get("info"), prob["f"],
                                 prob["cx"], prob["cy"])
    elif stereo:
        s.baSetStereoEdges(k, prob["cam_idx"], prob["pt_idx"], prob["meas"], None, prob["f"], prob["cx"], prob["cy"], prob["baseline"])
    else:
        s.baSetEdges(k, prob["cam_idx"], prob["pt_idx"], prob["meas"], None, prob["f"], prob["cx"], prob["cy"])
    pt_hidx = prob.get("pt_hidx")   # (a problem with fixed points carries its own landmark numbering)
    s.baSetEstimates(prob["cams"], prob["cam_hidx"], prob["pts"], np.arange(prob["L"], dtype=np.int32) if pt_hidx is None else pt_hidx)
    if pe is not None:
        s.baSetPoseEdges(kp, pe["vi"], pe["vj"], pe["meas"], pe.get("info"))
        if huber_delta_pose > 0:
            s.setRobustKernel(kp, capi.KERNEL_HUBER, huber_delta_pose)
    if huber_delta > 0:
        for kk in (s.psi_sets if psi else [k]):
            s.setRobustKernel(kk, capi.KERNEL_HUBER, huber_delta)
    return s, DeviceBAGraph(s)


def structure_only(solver, num_iters=10, num_max_trials=10, trace=False):
    """StructureOnlySolver<3>::calc(points, num_iters, num_max_trials) on the solver's bound projection set (ba_demo.cpp:261-269:
    the pre-step of the joint optimisation), every free point in one kernel launch.  trace=True returns (point_trace, point_chi2)
    of HipBlockSolver.baStructureOnly."""
    return solver.baStructureOnly(num_iters, num_max_trials, trace)


class DevicePoseGraph:
    """The graph protocol over HipBlockSolver's device-resident pose-graph front end (EdgeSE2 / EdgeSE3 / EdgeSim3, and the
    landmark observations bound beside them: setup_device_landmark_slam, setup_device_sim3_ba, setup_device_sbacam_ba)."""

    device_resident = True

    def __init__(self, solver):
        self.s = solver

    def linearize(self):
        self.s.pgLinearize(True)

    def compute_active_errors(self):
        self.s.pgLinearize(False)

    def chi2(self):
        return self.s.chi2()

    def update(self):
        self.s.pgUpdate()

    def push(self):
        self.s.pgPush()

    def pop(self):
        self.s.pgPop()

    def discard_top(self):
        self.s.pgDiscardTop()


PRIOR_ERROR_DIM = {7: 3, 8: 2, 9: 6}   # EdgeSE2Prior, EdgeSE2XYPrior, EdgeSE3Prior (g2ohip_pg_set_prior_edges)


PG_POSE_DIM = {1: 3, 2: 6, 10: 7}       # EdgeSE2, EdgeSE3, EdgeSim3 (g2ohip_pg_set_edges)


def setup_device_pose_graph(edge_type, estimates, hidx, num_free, vi, vj, meas, info, landmark_dim=None, device=0, priors=None,
                            fix_scale=False, options=None, offset_edges=None, calib_edges=None, huber_delta=0.0):
    """HipBlockSolver for a pose graph with estimates, errors and Jacobians on the device.
    edge_type 1: EdgeSE2 (estimates / measurements (x, y, theta), information [n][9]);
    edge_type 2: EdgeSE3 (isometries [12] = R column-major | t, information [n][36]).
    edge_type 10: EdgeSim3 over VertexSim3Expmap (estimates / measurements (qx, qy, qz, qw, tx, ty, tz, s), information
    [n][49]; BlockSolver_7_3); fix_scale: VertexSim3Expmap::_fix_scale of every vertex.  No priors beside this type.
    hidx[v] = hessian index of vertex v or -1 (fixed); BlockSolver_3_2 / BlockSolver_6_3 semantics, no Schur.
    options: g2ohip_set_option pairs that have to be in place before buildStructure.
    priors: (type, vq, zq, omega_q, offset) -- unary priors on the poses vq, type 7 = EdgeSE2Prior, 8 = EdgeSE2XYPrior
    (edge_type 1), 9 = EdgeSE3Prior with its ParameterSE3Offset or None (edge_type 2); solver.prior_set = their set id.
    offset_edges: (type, vi, vj, pfrom, pto, meas, info, offsets) -- pose-pose edges between sensor frames, type 18 =
    EdgeSE2Offset (edge_type 1), 19 = EdgeSE3Offset (edge_type 2), pfrom / pto rows of the offsets table (g2ohip_pg_set_offset_edges);
    solver.offset_set = their set id.
    calib_edges: dict(vi, vj, vl, meas, info) -- three-vertex EdgeSE2SensorCalib scan-match edges (edge_type 1 only): vi / vj the
    two poses, vl the laser offset, all rows of `estimates`; meas [n][3], info [n][9] or None (identity).  The three binary sets
    (i, j), (i, l), (j, l) are added with their parts and bound as one group (g2ohip_pg_set_sensor_calib_edges);
    solver.calib_sets = their ids; huber_delta > 0 puts a Huber kernel on all three.
    (EdgeSE2OdomDifferentialCalib edges: setup_device_odom_calib_graph.)"""
    return _setup_device_pose_graph(edge_type, estimates, hidx, num_free, vi, vj, meas, info, landmark_dim, device, priors, fix_scale,
                                    options, offset_edges, calib_edges, huber_delta, None)


def setup_device_odom_calib_graph(estimates, hidx, num_free, odom_calib_edges, vi=(), vj=(), meas=(), info=(), calib_edges=None,
                                  huber_delta=0.0, options=None, device=0):
    """setup_device_pose_graph(1, ...) for the graph of g2o/examples/calibration_odom_laser: the same arguments, and
    odom_calib_edges: dict(vi, vj, vp, meas, info) -- three-vertex EdgeSE2OdomDifferentialCalib edges: vi / vj the two poses, vp
    the VertexOdomDifferentialParams (k_l, k_r, b), all rows of `estimates` (the rows of vp are additive rows while the group is
    bound); meas [n][3] = (vl, vr, dt), info [n][9] or None (identity).  Added and bound like calib_edges
    (g2ohip_pg_set_odom_calib_edges), beside them or alone; solver.odom_calib_sets = their ids; huber_delta goes on these three
    too.  The EdgeSE2 set vi / vj / meas / info may be empty (the default): that example's graph holds no EdgeSE2."""
    return _setup_device_pose_graph(1, estimates, hidx, num_free, vi, vj, meas, info, None, device, None, False, options, None,
                                    calib_edges, huber_delta, odom_calib_edges)


def _setup_device_pose_graph(edge_type, estimates, hidx, num_free, vi, vj, meas, info, landmark_dim, device, priors, fix_scale, options,
                             offset_edges, calib_edges, huber_delta, odom_calib_edges):
    import numpy as np
    from . import capi
    d = PG_POSE_DIM[edge_type]
    s = capi.HipBlockSolver(d, landmark_dim or (2 if edge_type == 1 else 3), device)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    hidx = np.asarray(hidx, np.int32)
    k = s.addEdgeSet(d, hidx[np.asarray(vi, np.int64)], hidx[np.asarray(vj, np.int64)])
    if priors is not None:
        ptype, vq, zq, omega_q, offset = priors
        kq = s.addEdgeSet(PRIOR_ERROR_DIM[ptype], hidx[np.asarray(vq)], None)
    if offset_edges is not None:
        otype, oi, oj, opf, opt, omeas, oinfo, otable = offset_edges
        ko = s.addEdgeSet(d, hidx[np.asarray(oi, np.int64)], hidx[np.asarray(oj, np.int64)])
    if calib_edges is not None:
        ci, cj, cl = (np.asarray(calib_edges[key], np.int64) for key in ("vi", "vj", "vl"))
        parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
        kc = []
        for (a, b), pt in zip(((ci, cj), (ci, cl), (cj, cl)), parts):
            kc.append(s.addEdgeSet(3, hidx[a], hidx[b]))
            s.setEdgeSetParts(kc[-1], pt)
    if odom_calib_edges is not None:
        qi, qj, qp = (np.asarray(odom_calib_edges[key], np.int64) for key in ("vi", "vj", "vp"))
        parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
        kq3 = []
        for (a, b), pt in zip(((qi, qj), (qi, qp), (qj, qp)), parts):
            kq3.append(s.addEdgeSet(3, hidx[a], hidx[b]))
            s.setEdgeSetParts(kq3[-1], pt)
    s.buildStructure(num_free, 0, False)
    s.pgSetEdges(k, edge_type, vi, vj, meas, info)
    if edge_type == 10:
        s.pgSetSim3FixScale(fix_scale)
    s.pgSetEstimates(estimates, hidx)
    s.pose_set = k
    if priors is not None:
        s.pgSetPriorEdges(kq, ptype, vq, zq, omega_q, offset)
        s.prior_set = kq
    if offset_edges is not None:
        s.pgSetOffsetEdges(ko, otype, oi, oj, opf, opt, omeas, oinfo, otable)
    if calib_edges is not None:
        s.pgSetSensorCalibEdges(*kc, ci, cj, cl, calib_edges["meas"], calib_edges.get("info"))
        if huber_delta > 0:
            for kk in kc:
                s.setRobustKernel(kk, capi.KERNEL_HUBER, huber_delta)
    if odom_calib_edges is not None:
        s.pgSetOdomCalibEdges(*kq3, qi, qj, qp, odom_calib_edges["meas"], odom_calib_edges.get("info"))
        if huber_delta > 0:
            for kk in kq3:
                s.setRobustKernel(kk, capi.KERNEL_HUBER, huber_delta)
    return s, DevicePoseGraph(s)


def setup_device_landmark_slam(prob, huber_delta=0.0, schur=True, device=0, options=None):
    """HipBlockSolver for an openslam_g2o_amd.synthetic.make_landmark_slam (or g2o_io.landmark_problem) graph: odometry edges
    between poses (EdgeSE2 / EdgeSE3) plus observations of point landmarks (EdgeSE2PointXY / EdgeSE3PointXYZ, or -- when prob
    carries observation = "depth" | "disparity" and kcam -- EdgeSE3PointXYZDepth / EdgeSE3PointXYZDisparity), pose and
    landmark estimates, errors and Jacobians on the device; BlockSolver_3_2 / BlockSolver_6_3 semantics, landmarks
    marginalised (schur=True).  huber_delta > 0: Huber kernel on the observation set.  Returns (solver, DevicePoseGraph);
    solver.landmark_sets = (odometry set id, observation set id).  A prob that carries `prior` ("pose" | "xy", with vq, zq,
    omega_q and -- 3-D -- prior_offset) also gets its unary prior set bound (EdgeSE2Prior / EdgeSE2XYPrior / EdgeSE3Prior):
    solver.prior_set = its set id.  A prob of kind "se2" that carries bp, bl, zb and omega_b (synthetic.make_bearing_slam,
    g2o_io.bearing_problem) also gets its bearing-only observations bound (EdgeSE2PointXYBearing over the same landmark table):
    solver.bearing_set = their set id, huber_delta applies to them as well; the EdgeSE2PointXY set is then added only if
    prob["vp"] is present and non-empty (bearing-only SLAM otherwise: solver.landmark_sets = (odometry set id, None)).
    A prob of kind "se3" with observation = "stereo_vsc" and kcam = (fx, fy, cx, cy, baseline) (synthetic.make_scam_ba: the graph
    of g2o/examples/sba/sba_demo.cpp) has its observations bound as Edge_XYZ_VSC over VertexSCam cameras (pgSetScamEdges); the
    EdgeSE3 set vi / vj / Z / omega may be empty (the gauge is then held by fixed cameras or by priors).  If it also carries gi,
    gj, gmeas and ginfo (and gcov or None) -- the keys setup_device_gicp reads; the graph of g2o/examples/icp/gicp_sba_demo.cpp --
    the Edge_V_V_GICP correspondences are bound beside them on the same handle: solver.gicp_set = their set id (no kernel on
    them).  A prob that carries offset_edges = (19, vi, vj, pfrom, pto, meas, info, offsets) gets that EdgeSE3Offset set bound as
    well: solver.offset_set = its set id.
    A prob of kind "se2" that carries qp, ql, qc, zq and omega_q (synthetic.make_pointxy_calib_slam, g2o_io.pointxy_calib_problem;
    omega_q may be None = identity) also gets its EdgeSE2PointXYCalib edges bound: three-vertex edges over the pose qp, the
    landmark ql and the calibration vertex qc (a row of the pose table), added as the binary sets (pose, landmark), (pose, calib),
    (landmark, calib) with their parts (pgSetPointXYCalibEdges); solver.pointxy_calib_sets = their ids, huber_delta goes on all
    three; the EdgeSE2PointXY set is then added only if prob["vp"] is present and non-empty, as with bearings.  Such a prob must
    not carry `prior` as well (the priors' measurements use the keys zq / omega_q too): ValueError."""
    import numpy as np
    from . import capi
    se2 = prob["kind"] == "se2"
    bearing = se2 and all(prob.get(k) is not None for k in ("bp", "bl", "zb", "omega_b"))
    pcal = se2 and all(prob.get(k) is not None for k in ("qp", "ql", "qc"))
    if pcal and prob.get("prior") is not None:
        raise ValueError("setup_device_landmark_slam: a problem with pose priors and EdgeSE2PointXYCalib edges is not supported: "
                         "both read the keys zq / omega_q")
    with_xy = not (bearing or pcal) or (prob.get("vp") is not None and len(prob["vp"]) > 0)
    obs = prob.get("observation", "xyz")
    if obs in ("depth", "disparity") and prob.get("kcam") is None:
        raise ValueError("setup_device_landmark_slam: observation = %r needs kcam = (fx, fy, cx, cy)" % obs)
    scam = obs == "stereo_vsc"
    if scam and (se2 or prob.get("kcam") is None or np.asarray(prob["kcam"]).size != 5):
        raise ValueError("setup_device_landmark_slam: observation = 'stereo_vsc' needs kind 'se3' and kcam = (fx, fy, cx, cy, baseline)")
    gicp = scam and all(prob.get(k) is not None for k in ("gi", "gj", "gmeas", "ginfo"))
    offs = prob.get("offset_edges") if scam else None
    p, l = (3, 2) if se2 else (6, 3)
    s = capi.HipBlockSolver(p, l, device)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    hidx, pt_hidx = np.asarray(prob["hidx"], np.int32), np.asarray(prob["pt_hidx"], np.int32)
    k0 = s.addEdgeSet(p, hidx[prob["vi"]], hidx[prob["vj"]])
    k1 = s.addEdgeSet(l, hidx[prob["vp"]], pt_hidx[prob["vl"]]) if with_xy else None
    if bearing:
        kb = s.addEdgeSet(1, hidx[np.asarray(prob["bp"], np.int64)], pt_hidx[np.asarray(prob["bl"], np.int64)])
    if pcal:
        qp, ql, qc = (np.asarray(prob[k], np.int64) for k in ("qp", "ql", "qc"))
        parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
        kc3 = []
        for (a, b), pt in zip(((hidx[qp], pt_hidx[ql]), (hidx[qp], hidx[qc]), (pt_hidx[ql], hidx[qc])), parts):
            kc3.append(s.addEdgeSet(2, a, b))
            s.setEdgeSetParts(kc3[-1], pt)
    prior = prob.get("prior")
    if prior is not None:
        ptype = 9 if not se2 else (8 if prior == "xy" else 7)
        kq = s.addEdgeSet(PRIOR_ERROR_DIM[ptype], hidx[prob["vq"]], None)
    if gicp:
        kg = s.addEdgeSet(3, hidx[np.asarray(prob["gi"], np.int64)], hidx[np.asarray(prob["gj"], np.int64)])
    if offs is not None:
        ko = s.addEdgeSet(6, hidx[np.asarray(offs[1], np.int64)], hidx[np.asarray(offs[2], np.int64)])
    s.buildStructure(prob["nP"], prob["nL"], schur)
    if scam:   # (the EdgeSE3 set may be empty: its arrays still have their shapes)
        s.pgSetEdges(k0, 2, prob["vi"], prob["vj"], np.asarray(prob["Z"], np.float64).reshape(-1, 12),
                     np.asarray(prob["omega"], np.float64).reshape(-1, 36))
    else:
        s.pgSetEdges(k0, 1 if se2 else 2, prob["vi"], prob["vj"], prob["Z"], prob["omega"])
    s.pgSetEstimates(prob["poses"], hidx)
    if scam:
        s.pgSetScamEdges(k1, prob["vp"], prob["vl"], prob["zl"], prob["omega_l"], prob["kcam"])
        if gicp:
            s.pgSetGicpEdges(kg, prob["gi"], prob["gj"], prob["gmeas"], prob["ginfo"], prob.get("gcov"))
        if offs is not None:
            s.pgSetOffsetEdges(ko, *offs)
    elif obs in ("depth", "disparity"):
        s.pgSetLandmarkCameraEdges(k1, 5 if obs == "depth" else 6, prob["vp"], prob["vl"], prob["zl"], prob["omega_l"],
                                   prob.get("offset"), prob["kcam"])
    elif with_xy:
        s.pgSetLandmarkEdges(k1, 3 if se2 else 4, prob["vp"], prob["vl"], prob["zl"], prob["omega_l"], prob.get("offset"))
    if bearing:
        s.pgSetBearingEdges(kb, prob["bp"], prob["bl"], prob["zb"], prob["omega_b"])
    if pcal:
        s.pgSetPointXYCalibEdges(*kc3, qp, ql, qc, prob["zq"], prob.get("omega_q"))
    s.pgSetLandmarkEstimates(prob["points"], pt_hidx)
    if prior is not None:
        s.pgSetPriorEdges(kq, ptype, prob["vq"], prob["zq"], prob["omega_q"], prob.get("prior_offset"))
        s.prior_set = kq
    if huber_delta > 0 and with_xy:
        s.setRobustKernel(k1, capi.KERNEL_HUBER, huber_delta)
    if huber_delta > 0 and bearing:
        s.setRobustKernel(kb, capi.KERNEL_HUBER, huber_delta)
    if huber_delta > 0 and pcal:
        for k in kc3:
            s.setRobustKernel(k, capi.KERNEL_HUBER, huber_delta)
    s.landmark_sets = (k0, k1)
    return s, DevicePoseGraph(s)


def setup_device_sim3_ba(prob, huber_delta=0.0, schur=True, device=0, options=None):
    """HipBlockSolver for an openslam_g2o_amd.synthetic.make_sim3_ba (or g2o_io.sim3_ba_problem) graph: Sim3 keyframes
    (VertexSim3Expmap, EdgeSim3 between them -- possibly none) observing map points through EdgeSim3ProjectXYZ with per-camera
    intrinsics; pose and point estimates, errors and the numeric Jacobians on the device; BlockSolver_7_3 semantics, points
    marginalised (schur=True).  huber_delta > 0: Huber kernel on the observation set.  Returns (solver, DevicePoseGraph);
    solver.landmark_sets = (EdgeSim3 set id, observation set id), solver.pose_set = the former."""
    import numpy as np
    from . import capi
    s = capi.HipBlockSolver(7, 3, device)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    hidx, pt_hidx = np.asarray(prob["hidx"], np.int32), np.asarray(prob["pt_hidx"], np.int32)
    k0 = s.addEdgeSet(7, hidx[prob["vi"]], hidx[prob["vj"]])
    k1 = s.addEdgeSet(2, hidx[prob["vp"]], pt_hidx[prob["vl"]])
    s.buildStructure(prob["nP"], prob["nL"], schur)
    s.pgSetEdges(k0, 10, prob["vi"], prob["vj"], prob["meas"], prob["info"])
    s.pgSetSim3FixScale(prob.get("fix_scale", False))
    s.pgSetEstimates(prob["est"], hidx)
    s.pgSetSim3ProjectEdges(k1, prob["vp"], prob["vl"], prob["zl"], prob["omega_l"], prob["intrinsics"])
    s.pgSetLandmarkEstimates(prob["points"], pt_hidx)
    if huber_delta > 0:
        s.setRobustKernel(k1, capi.KERNEL_HUBER, huber_delta)
    s.landmark_sets = (k0, k1)
    s.pose_set = k0
    return s, DevicePoseGraph(s)


def setup_device_sbacam_ba(prob, huber_delta=0.0, schur=True, device=0, options=None, cam_huber_delta=0.0):
    """HipBlockSolver for an openslam_g2o_amd.synthetic.make_sbacam_ba (or g2o_io.sbacam_ba_problem) graph: bundle adjustment in
    the reference's SBA format -- VertexCam cameras with intrinsics and baselines of their own observing VertexSBAPointXYZ
    points through EdgeProjectP2MC (zl [m][2]) or EdgeProjectP2SC (zl [m][3]); camera and point estimates, errors and the
    analytic Jacobians on the device; BlockSolver_6_3 semantics, points marginalised (schur=True).  huber_delta > 0: Huber
    kernel on the observation set.  Optional prob["cam_edges"] / prob["scale_edges"] = dict(vi, vj, meas, info): EdgeSBACam
    (meas [n][7], info [n][36]) / EdgeSBAScale (meas [n], info [n]) constraints between cameras, each bound as a set of its own
    (pgSetCamEdges; the numeric Jacobians of the reference, on the device); cam_huber_delta > 0: Huber kernel on the
    EdgeSBACam set.  A problem with no points (no "vp", or an empty one) is a pure VertexCam pose graph: no observation set,
    no Schur complement.  Returns (solver, DevicePoseGraph); solver.landmark_sets = (the empty VertexCam set's id,
    observation set id or None), solver.pose_set = the former, solver.cam_set / solver.scale_set = the constraint sets' ids."""
    import numpy as np
    from . import capi
    s = capi.HipBlockSolver(6, 3, device)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    hidx = np.asarray(prob["hidx"], np.int32)
    with_points = len(prob.get("vp", ())) > 0
    none = np.zeros(0, np.int32)
    k0 = s.addEdgeSet(6, none, none)
    k1 = None
    if with_points:
        pt_hidx = np.asarray(prob["pt_hidx"], np.int32)
        zl = np.asarray(prob["zl"], np.float64)
        if zl.ndim != 2 or zl.shape[1] not in (2, 3):
            raise ValueError("setup_device_sbacam_ba: zl is [m][2] (EdgeProjectP2MC) or [m][3] (EdgeProjectP2SC)")
        d = zl.shape[1]
        k1 = s.addEdgeSet(d, hidx[prob["vp"]], pt_hidx[prob["vl"]])
    pose_sets = []
    for key, typ, dim in (("cam_edges", 16, 6), ("scale_edges", 17, 1)):
        e = prob.get(key)
        if e is not None:
            vi, vj = np.asarray(e["vi"], np.int32), np.asarray(e["vj"], np.int32)
            pose_sets.append((s.addEdgeSet(dim, hidx[vi], hidx[vj]), typ, vi, vj, e))
    if with_points:
        s.buildStructure(prob["nP"], prob["nL"], schur)
    else:
        s.buildStructure(prob["nP"], 0, False)
    s.pgSetEdges(k0, 12, none, none, np.zeros((0, 7)), np.zeros((0, 36)))
    s.pgSetEstimates(prob["est"], hidx)
    if with_points:
        s.pgSetCamProjectEdges(k1, 11 + d, prob["vp"], prob["vl"], zl, prob["omega_l"], prob["intrinsics"])
        s.pgSetLandmarkEstimates(prob["points"], pt_hidx)
        if huber_delta > 0:
            s.setRobustKernel(k1, capi.KERNEL_HUBER, huber_delta)
    for k, typ, vi, vj, e in pose_sets:
        s.pgSetCamEdges(k, typ, vi, vj, e["meas"], e["info"])
        if typ == 16 and cam_huber_delta > 0:
            s.setRobustKernel(k, capi.KERNEL_HUBER, cam_huber_delta)
    s.landmark_sets = (k0, k1)
    s.pose_set = k0
    return s, DevicePoseGraph(s)


def setup_device_gicp(prob, huber_delta=0.0, device=0, options=None):
    """HipBlockSolver for an openslam_g2o_amd.synthetic.make_gicp (or g2o_io.gicp_problem) graph: VertexSE3 scans joined by
    Edge_V_V_GICP correspondences (gi, gj, gmeas, ginfo and -- plane-to-plane -- gcov) and, optionally, EdgeSE3 odometry (vi, vj,
    Z, omega; empty arrays for a pure registration).  Poses, errors, the analytic Jacobians and the plane-to-plane information
    stay on the device; BlockSolver_6_3 semantics without landmarks.  huber_delta > 0: Huber kernel on the GICP set.  Returns
    (solver, DevicePoseGraph); solver.pose_set = the EdgeSE3 set's id, solver.gicp_set = the GICP set's."""
    import numpy as np
    from . import capi
    s = capi.HipBlockSolver(6, 3, device)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    hidx = np.asarray(prob["hidx"], np.int32)
    vi, vj = np.asarray(prob["vi"], np.int32), np.asarray(prob["vj"], np.int32)
    gi, gj = np.asarray(prob["gi"], np.int32), np.asarray(prob["gj"], np.int32)
    k0 = s.addEdgeSet(6, hidx[vi], hidx[vj])
    k1 = s.addEdgeSet(3, hidx[gi], hidx[gj])
    s.buildStructure(prob["nP"], 0, False)
    s.pgSetEdges(k0, 2, vi, vj, np.asarray(prob["Z"], np.float64).reshape(-1, 12), np.asarray(prob["omega"], np.float64).reshape(-1, 36))
    s.pgSetEstimates(prob["poses"], hidx)
    s.pgSetGicpEdges(k1, gi, gj, prob["gmeas"], prob["ginfo"], prob.get("gcov"))
    if huber_delta > 0:
        s.setRobustKernel(k1, capi.KERNEL_HUBER, huber_delta)
    s.pose_set = k0
    return s, DevicePoseGraph(s)
