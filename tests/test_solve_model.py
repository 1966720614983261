"""The fp64 model of the GN solve and the applied step (tests/solve_model.py) against the CPU oracle, on
photo_cases.make_photo_ba windows of nF = 2 ... 8 frames x 40 nF points at 160x120 (n = 20, 28, ..., 68).

The model is fed the oracle's own accumulate(0 / 1 / 2), prior and state, so what is compared is the solve alone.

Metrics (S = 1 / sqrt(diag HFinal + 10), the solve's own scaling, so x / S is the unknown the factorization sees):

    d_x   = ||(x - x64) / S||_inf / ||x64 / S||_inf
    d_blk = the largest ||dx||_2 / ||x64||_2 over the blocks calibration and, per frame, translation, rotation, a, b
            (a block whose entries are all below 1e-12 ||x64 / S||_inf S is skipped: a gauge-fixed or prior-pinned
            block that is 0 up to rounding has no relative error to speak of)

* d_oracle <= CEIL = 1e-6 for both metrics on every case (a condition on the cases, not a measurement); the floor
  n 2^-52 cond(S HFinal S) is printed beside it.
* every mutant of the model moves d_x or d_blk to >= 10 x CEIL (10 x the largest value the GPU bar can take) on at
  least one case that exercises it.  None is undetectable: lambda = 1e-5 moves H_sc by 2e-5 of itself, which the
  near-cancellation HA - H_sc amplifies well above 1e-5 in x (figures in DESIGN.md section 5).
* the model's gauge projector against the oracle's nullspaces() at 1e-9 of its largest entry.
* point_steps (H_fp, Hdd, bd of the photometric model, the oracle's x) against the oracle's points()["step"]:
  d_step = max |dstep| / ((|bd| + sum |H_fp x|) / Hdd) <= 1e-3 (fp64_model's cap for fp32-accumulated blocks).

Variants: photo_it0 (state = state_zero, no HM), fej_it1 / fej_it2 (photo_fej with a random PSD HM / bM: HM delta
live, orthogonalization off / on), calib_it2 (after one GN step under the weak calibration prior, HM / bM set:
calibration delta, bL's calibration rows and HM's calibration columns live), noid0_it2 (fej_it2 with every frame id
> 0: no strong first-frame prior in HL / bL; fej_it2 itself has the id-0 frame).
"""
import copy
import functools

import numpy as np
import pytest

import fp64_model as fm
import photo_cases as pc
import solve_model as sm

CEIL = 1e-6
STEP_CAP = 1e-3
NFS = list(range(2, 9))
# name: (kind, iteration, marginal prior, frame 0 keeps id 0)
VARIANTS = {"photo_it0": ("photo", 0, False, True), "fej_it1": ("photo_fej", 1, True, True),
            "fej_it2": ("photo_fej", 2, True, True), "calib_it2": ("calib", 2, True, True),
            "noid0_it2": ("photo_fej", 2, True, False)}
MUTANTS = {  # mutant: the variants that exercise it
    "hsc_times": list(VARIANTS), "lambda_on_hsc_diag": list(VARIANTS),
    "drop_HM_delta": ["fej_it1", "fej_it2", "calib_it2", "noid0_it2"],
    "drop_bL": ["photo_it0", "fej_it1", "fej_it2", "calib_it2"], "plus_bsc": list(VARIANTS),
    "orth_from_1": ["fej_it1"], "orth_raw_N": ["fej_it2", "calib_it2", "noid0_it2"], "calib_delta_sign": ["calib_it2"]}


# ------------------------------------------------------------------------------------------- shared with the GPU test
@functools.lru_cache(maxsize=None)
def scene_of(n_frames, kind, id0):
    s = pc.make_photo_ba(n_frames, 40 * n_frames, "photo" if kind == "calib" else kind)
    if not id0:
        s = copy.copy(s)
        s.frames_id = s.frames_id + 1
    return s


def params_of(kind, default_params):
    return pc.calib_params(default_params()) if kind == "calib" else None


def random_prior(HA, seed=3):
    """A random PSD HM / bM of the scale of the data Hessian (as test_gpu_ba.test_solve_with_marginal_prior)."""
    dim = len(HA)
    rng = np.random.default_rng(seed)
    Q = rng.normal(size=(dim, dim))
    HM = Q @ Q.T / dim * 1e-2 * np.abs(np.diag(HA)).mean()
    bM = rng.normal(size=dim) * 1e-2 * np.abs(HA).max() ** 0.5
    return HM, bM


def blocks(nF):
    out = [("calib", slice(0, 4))]
    for f in range(nF):
        r = 4 + 8 * f
        out += [(f"t{f}", slice(r, r + 3)), (f"r{f}", slice(r + 3, r + 6)), (f"a{f}", slice(r + 6, r + 7)),
                (f"b{f}", slice(r + 7, r + 8))]
    return out


def metrics(x, x64, S):
    """(d_x, d_blk, name of d_blk's block)."""
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    top = np.abs(x64 / S).max()
    d_x = float(np.abs((x - x64) / S).max() / top)
    d_blk, which = 0.0, None
    for name, sl in blocks((len(x) - 4) // 8):
        if np.all(np.abs(x64[sl]) < 1e-12 * top * S[sl]):
            continue
        d = float(np.linalg.norm(x[sl] - x64[sl]) / np.linalg.norm(x64[sl]))
        if d >= d_blk:
            d_blk, which = d, name
    return d_x, d_blk, which


def read_inputs(systems, HM, bM, frames, frame_eval, calib_zero, solverModeDelta):
    """The model's inputs from an engine's read-backs.  systems: which -> (H, b)."""
    (HA, bA), (HL, bL), (Hsc, bsc) = systems(0), systems(1), systems(2)
    delta = sm.stitched_delta(frames["state"], frame_eval["state_zero"], frames["calib"], calib_zero)
    return dict(HA=HA, bA=bA, HL=HL, bL=bL, Hsc=Hsc, bsc=bsc, HM=HM, bM=bM, delta=delta,
                N=sm.nullspaces(frame_eval["evalPT"]), solverModeDelta=solverModeDelta)


def model_x(inp, iteration, mutant=None):
    return sm.solve_x(iteration=iteration, mutant=mutant, **inp)


def system_figures(inp):
    """(S, cond(S HFinal S), the floor n 2^-52 cond)."""
    H, _ = sm.final_system(*[inp[k] for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc", "HM", "bM", "delta")])
    cond = sm.scaled_cond(H)
    return sm.scaling(H), cond, len(H) * 2.0 ** -52 * cond


def oracle_case_at(scene, cv, params, variant, prior=None):
    """The oracle on `scene` at calibration `cv`, linearized, with the variant's prior set: dict(o, inp, x, iteration,
    calib_zero, HM, bM).  prior: (HM, bM) to use (None: random_prior of the oracle's HA)."""
    from oracle_ffi import OracleBA
    _, iteration, with_prior, _ = VARIANTS[variant]
    o = OracleBA(scene, params=params)
    calib_zero = o.frames()["calib"].copy()          # right after the window is set: value_zero
    if cv is not None:
        o.set_calib(cv)
    o.linearize_all(reset=True)
    o.apply_res()
    dim = o.dim
    HM, bM = np.zeros((dim, dim)), np.zeros(dim)
    if with_prior:
        HM, bM = random_prior(o.accumulate(0)[0]) if prior is None else prior
        o.set_marginal_prior(HM, bM)
    inp = read_inputs(o.accumulate, HM, bM, o.frames(), o.frame_eval(), calib_zero, o.params.solverModeDelta)
    o.backup_state()
    x = o.solve_system(iteration)
    return dict(o=o, inp=inp, x=x, iteration=iteration, calib_zero=calib_zero, HM=HM, bM=bM, scene=scene, cv=cv)


@functools.lru_cache(maxsize=None)
def oracle_case(n_frames, variant):
    """The CPU case: 'calib' is the oracle's own state after one GN step under the weak calibration prior."""
    from oracle_ffi import default_params
    kind, _, _, id0 = VARIANTS[variant]
    s = scene_of(n_frames, kind, id0)
    params = params_of(kind, default_params)
    cv = None
    if kind == "calib":
        s, cv = pc.stepped(s, pc.oracle_at(s, params=params))
    return oracle_case_at(s, cv, params, variant)


def step_metric(step, scene, cv, active, x):
    """(d_step, model steps, has_active) of an engine's point steps at its own frame step x."""
    m = fm.ba_systems(scene, active, **pc.model_inputs(scene, cv))
    has = np.bincount(scene.res_point[np.asarray(active).astype(bool)], minlength=scene.n_points) > 0
    st64, scale = sm.point_steps(m["Hfp"], m["Hpp"], m["bp"], x, has)
    sel = scale > 0
    return float((np.abs(np.asarray(step, np.float64) - st64)[sel] / scale[sel]).max()), st64, has


CASES = [(nF, v) for nF in NFS for v in VARIANTS]


def case_id(c):
    return f"{c[0]}f-{c[1]}"


# ------------------------------------------------------------------------------------------- model against oracle
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_solve_model_against_oracle(case):
    c = oracle_case(*case)
    S, cond, floor = system_figures(c["inp"])
    x64 = model_x(c["inp"], c["iteration"])
    d_x, d_blk, which = metrics(c["x"], x64, S)
    print(f"{case_id(case)}: n {len(x64)}  cond {cond:.2e}  floor {floor:.2e}  d_oracle x {d_x:.2e}  "
          f"blocks {d_blk:.2e} ({which})")
    assert d_x <= CEIL and d_blk <= CEIL, (d_x, d_blk, which)
    assert np.array_equal(c["inp"]["Hsc"], c["inp"]["Hsc"].T)   # one symmetric H_sc: read back, solved, the device's
    kind, iteration, with_prior, id0 = VARIANTS[case[1]]
    # the variant is live where it says so
    if with_prior:
        assert np.abs(c["HM"] @ c["inp"]["delta"]).max() > 0
    if kind == "calib":
        assert np.abs(c["inp"]["delta"][:4]).min() > 0 and np.abs(c["inp"]["bL"][:4]).min() > 0
    HL = c["inp"]["HL"]
    assert (np.diag(HL)[4:10].min() > 0) == id0, np.diag(HL)[:12]


@pytest.mark.parametrize("n_frames", NFS)
def test_model_projector_against_oracle_nullspaces(n_frames):
    """The model's nullspaces (written from setStateZero / getNullspaces) span what the oracle's do: the projectors
    0.5 (N Npi^T + Npi N^T) agree at 1e-9 of their largest entry, and the model's N is the oracle's up to 1e-9."""
    c = oracle_case(n_frames, "fej_it2")
    o = c["o"]
    cut = o.params.solverModeDelta
    P64 = sm.projector(c["inp"]["N"], cut)
    Po = sm.projector(o.nullspaces().T, cut)
    assert np.abs(P64 - Po).max() <= 1e-9 * np.abs(P64).max()
    assert np.abs(c["inp"]["N"] - o.nullspaces().T).max() <= 1e-9 * np.abs(c["inp"]["N"]).max()
    assert np.linalg.matrix_rank(P64, tol=1e-6) == sm.NNS
    assert np.abs(P64 @ P64 - P64).max() <= 1e-12          # a projector


@functools.lru_cache(maxsize=None)
def mutant_figures(mutant):
    """[(case id, d_x, d_blk)] of the oracle's x against the mutated model on the variants that exercise it."""
    out = []
    for v in MUTANTS[mutant]:
        for nF in NFS:
            c = oracle_case(nF, v)
            S, _, _ = system_figures(c["inp"])
            if mutant == "calib_delta_sign":
                o, cz = c["o"], c["calib_zero"]
                dl = sm.stitched_delta(o.frames()["state"], o.frame_eval()["state_zero"], o.frames()["calib"], cz,
                                       mutant=mutant)
                xm = model_x(dict(c["inp"], delta=dl), c["iteration"])
            else:
                xm = model_x(c["inp"], c["iteration"], mutant=mutant)
            d_x, d_blk, _ = metrics(c["x"], xm, S)
            out.append((case_id((nF, v)), d_x, d_blk))
    return out


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_solve_mutants_clear_the_bar(mutant):
    figs = mutant_figures(mutant)
    worst = max(figs, key=lambda f: max(f[1], f[2]))
    least = min(figs, key=lambda f: max(f[1], f[2]))
    print(f"{mutant}: largest d {max(worst[1:]):.2e} ({worst[0]}), smallest {max(least[1:]):.2e} ({least[0]}) over "
          f"{len(figs)} cases")
    assert max(worst[1:]) >= 10 * CEIL, figs


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_point_steps_against_oracle(case):
    c = oracle_case(*case)
    o = c["o"]
    active = o.residuals()["state"] == 0
    d, st64, has = step_metric(o.points()["step"], c["scene"], c["cv"], active, c["x"])
    print(f"{case_id(case)}: points with an active residual {int(has.sum())}/{len(has)}  d_oracle step {d:.2e}")
    assert has.sum() >= 4 and d <= STEP_CAP, d
    assert np.all(o.points()["step"][~has] == 0)


def test_apply_step_against_oracle():
    """doStepFromBackup on the oracle against apply_step: state and calibration exactly (one fp64 add each), the pose
    within 1e-12, idepth = float32(idepth + step)."""
    for case in [(2, "photo_it0"), (5, "calib_it2"), (8, "fej_it2")]:
        k = oracle_case(*case)      # shared and left as it is: the step is taken on a fresh oracle at the same state
        c = oracle_case_at(k["scene"], k["cv"], k["o"].params, case[1], prior=(k["HM"], k["bM"]))
        assert np.array_equal(c["x"], k["x"])
        o = c["o"]
        before, ev = o.frames(), o.frame_eval()["evalPT"]
        idp, step = o.points()["idepth"].copy(), o.points()["step"].copy()
        o.do_step()
        after = o.frames()
        new, poses, calib = sm.apply_step(before["state"], c["x"], ev, before["calib"])
        assert np.array_equal(after["state"], new) and np.array_equal(after["calib"], calib)
        for f, (R, t) in enumerate(poses):
            Ro, to = fm.se3_from_data(after["pose"][f])
            assert np.abs(Ro - R).max() <= 1e-12 and np.abs(to - t).max() <= 1e-12
        assert np.array_equal(o.points()["idepth"], (idp + step).astype(np.float32))
