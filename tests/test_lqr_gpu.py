"""CACLA on LQR on the fused kernel (sw_lqr_cacla_run_f64) on the GPU: drop-in parity with the reference's own runs
(tests/golden/lqr.npz), batches, split runs, runs without records and a diverging agent.

Bounds: 1e-9 absolute against the reference's goldens -- the project's standing bound for runs of <= 1000 steps
(tests/test_hip_parity.py); shapes, counters, the random-stream witness, batch rows and split runs are compared
exactly."""
import os

import numpy as np
import pytest

import swimmer_amd as sw
from conftest import GOLDEN, observed
from swimmer_amd import cacla
from swimmer_amd.cacla import cacla_safe_agent, lqr
from swimmer_amd.envs.gym_lqr import lqr_env

import lqr_oracle

pytestmark = pytest.mark.gpu

CASES = tuple(lqr_oracle.CASES)
_seen = {}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "lqr.npz"), allow_pickle=False)


@pytest.mark.parametrize("tag", CASES)
def test_drop_in_against_the_reference(gold, tag):
    case = lqr_oracle.CASES[tag]
    agent, real, sim = lqr_oracle.build(case, lqr_env, cacla.CACLA_LQR_agent, cacla_safe_agent)
    np.random.seed(case["seed"])
    got = agent.run(case["steps"], case["gamma"], case["alpha"], case["sigma"])
    fig = {}
    for name, g in zip(("states", "actions", "rewards"), got):
        want = gold[f"{tag}_{name}"]
        assert isinstance(g, np.ndarray) and g.shape == want.shape, (name, g.shape, want.shape)
        fig[name] = float(np.abs(g - want).max()) if want.size else 0.0
    fig["F"] = float(np.abs(agent.F - gold[f"{tag}_F"]).max())
    fig["V"] = float(np.abs(agent.V - gold[f"{tag}_V"]).max())
    fig["state"] = float(np.abs(np.asarray(real.state) - gold[f"{tag}_state"]).max())
    _seen[tag] = fig
    observed("lqr_parity", _seen)
    assert [agent.admitted, agent.violations, agent.actor_updates] == gold[f"{tag}_counters"].tolist()
    assert agent.status == 0
    assert np.random.standard_normal() == gold[f"{tag}_next_normal"]     # the global stream is where the reference's is
    assert max(fig.values()) <= 1e-9, fig


def test_progress_lines_are_the_references(gold, capsys):
    """Every H steps the last admitted reward; nothing while nothing has been admitted (L32: 33 leading refusals)."""
    for tag, H in (("P11", 250), ("L32", 20)):
        case = lqr_oracle.CASES[tag]
        agent, _, _ = lqr_oracle.build(case, lqr_env, cacla.CACLA_LQR_agent, cacla_safe_agent)
        np.random.seed(case["seed"])
        capsys.readouterr()
        _, _, rewards = agent.run(case["steps"], case["gamma"], case["alpha"], case["sigma"], H=H)
        lines = capsys.readouterr().out.splitlines()
        skipped = case["steps"] - len(rewards)
        want = [f"Iteration {i}/{case['steps']}: reward: {rewards[i - skipped]}"
                for i in range(H, case["steps"], H) if i >= skipped]
        assert lines == want and len(want) == {"P11": 3, "L32": 11}[tag]


def test_f_and_v_are_kept_across_runs(gold):
    """A second run() continues from the learnt F and V (a fresh initial state and fresh noise), as the reference's."""
    case = lqr_oracle.CASES["P12"]
    agent, real, _ = lqr_oracle.build(case, lqr_env, cacla.CACLA_LQR_agent, cacla_safe_agent)
    np.random.seed(case["seed"])
    agent.run(300, case["gamma"], case["alpha"], case["sigma"])
    F1, V1 = agent.F.copy(), agent.V.copy()
    stream = np.random.get_state()
    x0 = np.random.rand(2)                                       # what the second run is going to draw
    noise = np.random.multivariate_normal(np.zeros(1), case["sigma"] * np.identity(1), size=200)
    np.random.set_state(stream)
    states, actions, rewards = agent.run(200, case["gamma"], case["alpha"], case["sigma"])
    want = lqr_oracle.run(lqr_oracle.model(real), real.Q, real.R, case["gamma"], case["alpha"], x0, noise, F0=F1, V0=V1)
    assert np.array_equal(states[0], x0)
    assert np.abs(rewards - want["rewards"]).max() <= 1e-9 and np.abs(agent.F - want["F"]).max() <= 1e-9
    assert np.abs(agent.V - want["V"]).max() <= 1e-9 and agent.actor_updates == want["actor_updates"]


def _mixed(A):
    k = np.arange(A)
    return dict(theta=np.linspace(0.8, 1.0, A), theta_sim=np.linspace(0.78, 0.97, A),
                gammas=np.array([1.0, 0.9, 0.5])[k % 3], alphas=np.array([1e-2, 3e-3, 1e-3, 1e-4, 5e-3])[k % 5],
                sigmas=np.array([1.0, 0.1, 0.3, 0.01])[k % 4], ls=np.array([1.5, 1.0, 4.0, 0.7, 2.0])[(k // 2) % 5],
                seeds=list(range(200, 200 + A)))


@pytest.mark.parametrize("kind", ("plain", "se"))
def test_batch_rows_are_independent_agents_bit_for_bit(kind):
    """67 agents: one full wave and three lanes of a second one."""
    A, steps = 67, 100
    m = _mixed(A)
    reals = [lqr_env.EasyParamLinearQuadReg(t) for t in m["theta"]]
    sims = [lqr_env.EasyParamLinearQuadReg(t) for t in m["theta_sim"]]
    cons = [cacla_safe_agent.Constraint(lambda x: np.linalg.norm(x, np.inf), l, 1) for l in m["ls"]]
    eps = np.abs(m["theta"] - m["theta_sim"])

    def batch(n):
        safe = {} if kind == "plain" else dict(sim_envs=sims[:n], epsilons=eps[:n], constraints=cons[:n])
        b = cacla.CACLA_LQR_Batch(reals[:n], m["gammas"][:n], m["alphas"][:n], m["sigmas"][:n], m["seeds"][:n],
                                  agent=kind, **safe)
        return b, b.run(steps)
    before = np.random.get_state()[1].copy()
    small, r3 = batch(3)
    big, r67 = batch(A)
    assert np.array_equal(np.random.get_state()[1], before)          # the global stream is not touched
    assert r67["states"].shape == (A, steps, 2) and r67["actions"].shape == (A, steps, 1)
    assert r67["rewards"].shape == (A, steps) and r67["admitted"].shape == (A, steps)
    assert big.F.shape == (A, 1, 2) and big.V.shape == (A, 2) and big.state.shape == (A, 2)
    assert not big.status.any()
    if kind == "se":        # the batch is not all of one fate: refusals and admissions, leading refusals too
        assert big.admitted.min() < steps and (big.admitted == steps).any()
        assert (r67["admitted"] == sw.kernels.LQR_NOTHING_YET).any() and (r67["admitted"] == sw.kernels.LQR_REFUSED).any()
    else:
        assert (big.admitted == steps).all() and (r67["admitted"] == sw.kernels.LQR_ADMITTED).all()
    assert big.actor_updates.max() > 0
    for a in (0, 1, 63, 64, 66):
        np.random.seed(m["seeds"][a])
        if kind == "plain":
            agent = cacla.CACLA_LQR_agent(reals[a])
        else:
            agent = cacla_safe_agent.CACLA_LQR_SE_agent(reals[a], sims[a], eps[a], cons[a])
        got = agent.run(steps, m["gammas"][a], m["alphas"][a], m["sigmas"][a])
        for g, w in zip(got, big.arrays_of(a)):
            assert g.shape == w.shape and np.array_equal(g, w), a
        assert np.array_equal(agent.F, big.F[a]) and np.array_equal(agent.V, big.V[a])
        assert np.array_equal(np.asarray(reals[a].state), big.state[a])
        assert (agent.admitted, agent.violations, agent.actor_updates, agent.status) == \
            (big.admitted[a], big.violations[a], big.actor_updates[a], big.status[a])
    for name in r3:
        assert np.array_equal(r3[name], r67[name][:3]), name
    assert np.array_equal(small.F, big.F[:3]) and np.array_equal(small.V, big.V[:3])
    assert np.array_equal(small.admitted, big.admitted[:3]) and np.array_equal(small.actor_updates, big.actor_updates[:3])


def _runner(kind, columns, cost, x0, noise):
    """A lqr.Run of the given agents, and a draw() that hands out the prepared noise [A, T, na] piece by piece."""
    A, T, na = noise.shape
    ns = x0.shape[1]
    run = lqr.Run(kind, ns, na, cost, np.stack(columns), np.zeros((A, na, ns)), np.zeros((A, ns)), x0)
    at = [0]

    def draw(c):
        at[0] += c
        return noise[:, at[0] - c:at[0]]
    return run, draw


def _in_parts(kind, columns, cost, x0, noise, parts):
    run, draw = _runner(kind, columns, cost, x0, noise)
    recs = [run.run(c, c, draw) for c in parts]
    rec = {k: np.concatenate([r[k] for r in recs], axis=1) for k in recs[0]}
    return rec, run.finals()


@pytest.mark.parametrize("kind", ("plain", "se"))
def test_splitting_a_run_changes_nothing(kind):
    """100 steps in one launch, as 37 + 63 and as 64 + 36: lengths that are no multiple of the noise block."""
    A, steps = 5, 100
    m = _mixed(A)
    cons = [cacla_safe_agent.Constraint(cacla.norm_cost(np.inf), l, 1) for l in m["ls"]]
    cols, cost = [], None
    for a in range(A):
        col, cost = lqr.agent_column(kind, lqr_env.EasyParamLinearQuadReg(m["theta"][a]), m["gammas"][a],
                                     m["alphas"][a], lqr_env.EasyParamLinearQuadReg(m["theta_sim"][a]),
                                     abs(m["theta"][a] - m["theta_sim"][a]), cons[a])
        cols.append(col)
    rs = np.random.RandomState(17)
    x0 = rs.rand(A, 2)
    noise = rs.normal(0.0, np.sqrt(m["sigmas"])[:, None, None], size=(A, steps, 1))
    whole_rec, whole_fin = _in_parts(kind, cols, cost, x0, noise, [steps])
    assert whole_fin[5].sum() > 0 and not whole_fin[6].any() and whole_fin[3].min() > 0
    if kind == "se":
        assert whole_fin[3].min() < steps
    for parts in ([37, 63], [64, 36]):
        rec, fin = _in_parts(kind, cols, cost, x0, noise, parts)
        for k in whole_rec:
            assert np.array_equal(whole_rec[k], rec[k]), (parts, k)
        for a, b in zip(whole_fin, fin):
            assert np.array_equal(a, b), parts


def test_a_split_inside_the_leading_refusals(gold):
    """L32 refuses its first 33 steps: 20 + 236 hands 'nothing admitted yet' from one launch to the next."""
    case = lqr_oracle.CASES["L32"]
    agent, real, sim = lqr_oracle.build(case, lqr_env, cacla.CACLA_LQR_agent, cacla_safe_agent)
    col, cost = lqr.agent_column("se", real, case["gamma"], case["alpha"], sim, lqr_oracle.epsilon_of(case),
                                 agent.constraint)
    x0, noise = gold["L32_x0"][None], gold["L32_noise"][None]
    whole_rec, whole_fin = _in_parts("se", [col], cost, x0, noise, [256])
    rec, fin = _in_parts("se", [col], cost, x0, noise, [20, 236])
    for k in whole_rec:
        assert np.array_equal(whole_rec[k], rec[k]), k
    for a, b in zip(whole_fin, fin):
        assert np.array_equal(a, b)
    assert (rec["admitted"][0, :33] == sw.kernels.LQR_NOTHING_YET).all() and rec["admitted"][0, 33] == 1
    states, actions, rewards = lqr.reference_arrays(rec["states"][0], rec["actions"][0], rec["rewards"][0],
                                                    rec["admitted"][0])
    assert states.shape == (223, 2) and np.abs(states - gold["L32_states"]).max() <= 1e-9
    assert np.abs(rewards - gold["L32_rewards"]).max() <= 1e-9 and np.abs(actions - gold["L32_actions"]).max() <= 1e-9
    assert [fin[3][0], fin[4][0], fin[5][0]] == gold["L32_counters"].tolist()


@pytest.mark.parametrize("kind", ("plain", "bounded"))
def test_without_records_the_finals_are_the_same(kind):
    A, steps = 70, 150
    m = _mixed(A)
    if kind == "plain":
        args = dict(agent="plain")
        reals = [lqr_env.EasyParamLinearQuadReg(t) for t in m["theta"]]
    else:
        reals = [lqr_env.BoundedEasyLinearQuadReg(t, 2.0, 1.0) for t in m["theta"]]
        args = dict(agent="bounded", sim_envs=[lqr_env.BoundedEasyLinearQuadReg(t, 2.0, 1.0) for t in m["theta_sim"]],
                    epsilons=np.abs(m["theta"] - m["theta_sim"]),
                    constraints=cacla_safe_agent.Constraint(cacla.norm_cost(np.inf), 1.5, 1))
    full = cacla.CACLA_LQR_Batch(reals, m["gammas"], m["alphas"], m["sigmas"], m["seeds"], **args)
    none = cacla.CACLA_LQR_Batch(reals, m["gammas"], m["alphas"], m["sigmas"], m["seeds"], **args)
    some = cacla.CACLA_LQR_Batch(reals, m["gammas"], m["alphas"], m["sigmas"], m["seeds"], **args)
    rec = full.run(steps, chunk=64)
    assert none.run(steps, chunk=64, record=()) == {}
    only = some.run(steps, chunk=64, record=("rewards",))
    assert list(only) == ["rewards"] and np.array_equal(only["rewards"], rec["rewards"])
    for b in (none, some):
        for name in ("F", "V", "state", "admitted", "violations", "actor_updates", "status"):
            assert np.array_equal(getattr(full, name), getattr(b, name)), name
    assert full.actor_updates.sum() > 0 and (full.admitted > 0).all()
    with pytest.raises(ValueError):
        full.run(steps, record=("reward",))


def test_a_diverging_agent_stays_contained():
    """The plain agent of seed 2 with alpha = 0.1 on the reference's instance 2 overflows (in the reference too: its
    rewards are -inf from step 1185 and NaN from step 2304); its neighbours in the batch do not notice."""
    env, steps = lqr_oracle.make_env(lqr_env, "lqr2"), 2560
    with_it = cacla.CACLA_LQR_Batch(env, 1, [0.01, 0.1, 0.01], 0.1, [1, 2, 3])
    r = with_it.run(steps, record=("rewards",))["rewards"]
    without = cacla.CACLA_LQR_Batch(env, 1, [0.01, 0.01], 0.1, [1, 3])
    r2 = without.run(steps, record=("rewards",))["rewards"]
    assert with_it.status[1] & sw._lib.STATUS_NONFINITE
    nan = np.flatnonzero(np.isnan(r[1]))
    assert nan.size and np.isnan(r[1][nan[0]:]).all() and np.isfinite(r[1][:1000]).all(), nan[:4]
    assert with_it.status[0] == 0 and with_it.status[2] == 0
    assert np.array_equal(r[[0, 2]], r2) and np.isfinite(r2).all()
    for name in ("F", "V", "state", "admitted", "actor_updates"):
        assert np.array_equal(getattr(with_it, name)[[0, 2]], getattr(without, name)), name
    assert with_it.actor_updates[1] < with_it.admitted[1] == steps      # a NaN temporal difference updates no actor


def test_experiment_functions(tmp_path):
    """sweep() and compare() on small runs: rows are the single agents, figures are written on Agg."""
    out = cacla.lqr_experiment.sweep(alphas=(0.01, 0.001), n_iter=400, H=100, out_dir=str(tmp_path / "sweep"))
    assert len(out["curves"]) == 2 and out["curves"][0].shape == (300,) and out["t"].shape == (300,)
    np.random.seed(1)
    agent = cacla.CACLA_LQR_agent(cacla.lqr_experiment.lqr_2())
    _, _, rewards = agent.run(400, 1, 0.001, 0.1)
    assert np.array_equal(out["F"][1], agent.F)
    assert np.array_equal(out["curves"][1], cacla.window_convolution(rewards, 100))
    assert out["distance"][1] == float(np.linalg.norm(agent.F - cacla.lqr_experiment.OPTIMAL_F))
    both = cacla.safe_exploration_lqr.compare(n_iter=600, H=100, seed=9, out_dir=str(tmp_path / "cmp"))
    np.random.seed(9)
    plain = cacla.CACLA_LQR_agent(lqr_env.EasyAffineQuadReg(1.0))
    s1 = plain.run(600, 1, 0.0001, 0.1)
    np.random.seed(9)
    safe = cacla_safe_agent.CACLA_AffineQR_SE_agent(
        lqr_env.EasyAffineQuadReg(1.0), lqr_env.EasyAffineQuadReg(0.99), abs(1.0 - 0.99),
        cacla_safe_agent.Constraint(lambda x: np.linalg.norm(x, np.inf), 4, 1))
    s2 = safe.run(600, 1, 0.0001, 0.1)
    for name, got, agent_ in (("plain", s1, plain), ("safe", s2, safe)):
        for k, g in zip(("states", "actions", "rewards"), got):
            assert np.array_equal(both[name][k], g), (name, k)
        assert np.array_equal(both[name]["F"], agent_.F)
    assert both["safe"]["admitted"] == safe.admitted < 600 == both["plain"]["admitted"]
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    assert len(list((tmp_path / "sweep").glob("*.png"))) == 3 and len(list((tmp_path / "cmp").glob("*.png"))) == 1
