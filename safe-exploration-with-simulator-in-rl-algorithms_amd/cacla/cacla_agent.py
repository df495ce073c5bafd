"""CACLA with neural-network function approximators (cacla/cacla_agent.py:19-58, :135-199) on the fused kernel.

The learner itself -- actor forward, Gaussian action, physics step, the two critic evaluations, the SGD step on the
critic and the conditional one on the actors -- runs on the GPU for whole chunks of steps (kernels.cacla_run).  What
stays on the host is what fixes the random streams: the initial weights are drawn as the reference draws them
(torch.nn.Linear's initialisation, actor networks first, then the critic) and the exploration noise comes from
NumPy's legacy multivariate_normal, chunk by chunk: `multivariate_normal(zeros, sigma I, size=c)` consumes the stream
exactly as c of the reference's per-step calls `multivariate_normal(FA_act, sigma I)` do and returns their noise
(the mean is added last there, and in the kernel).  `sigma` is the VARIANCE of the policy, as in the reference.

One network is a vector of net_doubles(n) doubles, W1 [12][d] row-major | b1 [12] | W2 [12] | b2 (the layout of
include/swimmer_hip.h); an agent is its n - 1 actor networks followed by the critic.
"""
import math

import numpy as np
import torch

from .. import kernels
from .._lib import STATUS_SINGULAR, SwimmerHipError, dev_f64

HIDDEN = kernels.CACLA_HIDDEN


def net_doubles(n):
    return kernels.cacla_net_doubles(n)


def pack_net(w1, b1, w2, b2):
    """linear1.weight [12, d], linear1.bias [12], linear2.weight [1, 12] or [12], linear2.bias -> one network."""
    return np.concatenate([np.asarray(w1, dtype=np.float64).reshape(-1), np.asarray(b1, dtype=np.float64).reshape(-1),
                           np.asarray(w2, dtype=np.float64).reshape(-1), np.asarray(b2, dtype=np.float64).reshape(-1)])


def unpack_net(vec, d):
    """One network -> (W1 [12, d], b1 [12], W2 [12], b2)."""
    vec = np.asarray(vec)
    a, b = HIDDEN * d, HIDDEN * d + HIDDEN
    return vec[:a].reshape(HIDDEN, d), vec[a:b], vec[b:b + HIDDEN], vec[b + HIDDEN]


def _linear(n_in, n_out, generator):
    """The parameters of torch.nn.Linear(n_in, n_out).double() as float64 arrays.  generator None: the module itself,
    from torch's global generator; otherwise Linear.reset_parameters' two draws from `generator`."""
    if generator is None:
        lin = torch.nn.Linear(n_in, n_out).double()
        return lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()
    w, b = torch.empty(n_out, n_in), torch.empty(n_out)
    torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5), generator=generator)
    bound = 1 / math.sqrt(n_in)
    torch.nn.init.uniform_(b, -bound, bound, generator=generator)
    return w.double().numpy(), b.double().numpy()


def draw_networks(n, generator=None):
    """The n networks of a fresh agent, [n, net_doubles(n)], in the order CACLA_agent.run creates them
    (cacla_agent.py:165-166): ActorFA's n - 1 TwoLayersNet(d, 12), then CriticFA's; within a net linear1, linear2."""
    d = 2 * n + 2
    nets = np.empty((n, net_doubles(n)))
    for k in range(n):
        w1, b1 = _linear(d, HIDDEN, generator)
        w2, b2 = _linear(HIDDEN, 1, generator)
        nets[k] = pack_net(w1, b1, w2, b2)
    return nets


class Uploader(object):
    """Double-buffered upload of host chunks (float64 arrays of at most max_elems elements): chunk k + 1 is drawn
    into one pinned buffer while the copy of chunk k leaves the other and its launch runs (copies and launches are
    asynchronous on the current stream).  Shared by the swimmer's and the LQR agents' chunk loops."""

    def __init__(self, max_elems, device):
        self.device = device
        self.host = [torch.empty(max_elems, dtype=torch.float64).pin_memory() for _ in range(2)]
        self.copied = [None, None]
        self.k = 0

    def upload(self, array):
        i = self.k % 2
        self.k += 1
        if self.copied[i] is not None:
            self.copied[i].synchronize()          # its last upload has left the pinned buffer
        view = self.host[i][:array.size].view(array.shape)
        view.numpy()[...] = array
        out = view.to(self.device, non_blocking=True)
        self.copied[i] = torch.cuda.Event()
        self.copied[i].record()
        return out


def chunk_sizes(n_iter, chunk):
    """The steps of each launch of a run of n_iter steps, at most `chunk` per launch."""
    if n_iter < 0 or chunk < 1:
        raise SwimmerHipError("n_iter must be >= 0 and chunk >= 1")
    return [min(chunk, n_iter - t) for t in range(0, n_iter, chunk)]


def run_chunks(device, A, m, sizes, draw, launch):
    """The chunk loop of a run of A agents, plain or gated.  draw(c) returns the next c steps' noise [A, c, m] on the
    host; launch(c, t, noise) starts the c steps from step t on with that noise on the device and returns the
    chunk's per-step outputs, a tuple of [A, c] device tensors.  Chunk k + 1 is drawn while chunk k runs (launches
    are asynchronous), and the outputs come back in one copy each at the end: a list of [A, sum(sizes)] arrays."""
    outs, t = [], 0
    with torch.cuda.device(device):
        up = Uploader(A * max(sizes) * m, device)
        for c in sizes:
            outs.append(launch(c, t, up.upload(np.asarray(draw(c), dtype=np.float64).reshape(A, c, m))))
            t += c
        return [(col[0] if len(col) == 1 else torch.cat(col, dim=1)).cpu().numpy() for col in zip(*outs)]


def draw_batch(env, seeds, sigmas):
    """What fixes the random streams of a batch: agent a's initial weights from torch.Generator().manual_seed(seeds[a])
    and its noise from np.random.RandomState(seeds[a]) with variance sigmas[a], as the single classes draw theirs
    from the global generators after seeding both with seeds[a].  -> (weights [A, n, net_doubles(n)], draw, the reset
    state once per agent [A, d]); draw(c) is the next c steps' noise [A, c, m]."""
    n, m = env.n, env.n - 1
    weights = np.stack([draw_networks(n, torch.Generator().manual_seed(s)) for s in seeds])
    streams = [np.random.RandomState(s) for s in seeds]
    covs = [s * np.identity(m) for s in sigmas]
    state = np.asarray(env.reset(), dtype=np.float64)
    zeros = np.zeros(m)

    def draw(c):
        return np.stack([rs.multivariate_normal(zeros, cov, size=c) for rs, cov in zip(streams, covs)])

    return weights, draw, np.tile(state, (len(seeds), 1))


class _Run(object):
    """The device side of a run of A agents: weights, state and counters.  run() is run_chunks() over
    kernels.cacla_run; draw(c) returns the next c steps' noise [A, c, m] on the host."""

    def __init__(self, p, device, gammas, alphas, weights, state):
        self.p, self.device = p, torch.device(device)
        A = len(gammas)
        self.A = A
        self.gamma = dev_f64(np.asarray(gammas, dtype=np.float64), self.device)
        self.alpha = dev_f64(np.asarray(alphas, dtype=np.float64), self.device)
        self.weights = dev_f64(weights, self.device)
        self.state = dev_f64(state, self.device)
        self.status = torch.zeros(A, dtype=torch.int32, device=self.device)
        self.actor_updates = torch.zeros(A, dtype=torch.int32, device=self.device)

    def run(self, n_iter, chunk, train, draw):
        sizes = chunk_sizes(n_iter, chunk)
        if not sizes:
            return np.empty((self.A, 0))
        if not train:
            # the actors keep seeing the observation the LAUNCH started from (include/swimmer_hip.h): one launch
            sizes = [n_iter]

        def launch(c, t, noise):
            return (kernels.cacla_run(self.p, c, train, self.gamma, self.alpha, noise, self.weights, self.state,
                                      actor_updates=self.actor_updates, status=self.status),)

        return run_chunks(self.device, self.A, self.p.m, sizes, draw, launch)[0]


class CACLA_agent:
    """Drop-in for the reference's CACLA_agent (cacla_agent.py:135-199); `env` is a swimmer_amd.SwimmerEnv.

    After run(): actor_weights [n - 1, net_doubles(n)], critic_weights [net_doubles(n)] (pack_net's layout; the
    initial ones when train=False), status (SW_STATUS_* bits OR-ed over the run) and actor_updates (steps with
    temp_diff > 0)."""

    chunk = 2048   # steps per launch

    def __init__(self, gamma, alpha, sigma):
        self.gamma = gamma
        self.alpha = alpha
        self.sigma = sigma
        self.actor_weights = self.critic_weights = self.initial_weights = None
        self.status = 0
        self.actor_updates = 0

    def run(self, env, n_iter, H=1000, train=True, render=False):
        n, m = env.n, env.n - 1
        assert env.observation_space.shape[0] == 2 * n + 2 and env.action_space.shape[0] == m
        weights = draw_networks(n)                                   # torch's global generator
        self.initial_weights = weights.copy()
        state = np.asarray(env.reset(), dtype=np.float64)
        cov = self.sigma * np.identity(m)
        run = _Run(env._params(), env.device, [self.gamma], [self.alpha], weights[None], state[None])
        rewards = run.run(int(n_iter), self.chunk, bool(train),
                          lambda c: np.random.multivariate_normal(np.zeros(m), cov, size=c)[None])[0]
        w = run.weights.cpu().numpy()[0]
        self.actor_weights, self.critic_weights = w[:m].copy(), w[m].copy()
        self.status = int(run.status.cpu()[0])
        self.actor_updates = int(run.actor_updates.cpu()[0])
        if self.status & STATUS_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")           # numpy.linalg.solve's, inside env.step
        env.set_state(run.state.cpu().numpy()[0].tolist())           # the environment has taken n_iter steps
        for i in range(H, n_iter, H):
            print(f"Iteration {i}/{n_iter}: reward: {rewards[i]}")
        return list(rewards)


class CACLABatch(object):
    """A independent CACLA agents on one SwimmerEnv's model, ONE launch per chunk of steps for all of them.

    Agent a has (gammas[a], alphas[a], sigmas[a]) and draws its initial weights from
    torch.Generator().manual_seed(seeds[a]) and its noise from np.random.RandomState(seeds[a]): row a of run() is,
    bit for bit, what CACLA_agent(gammas[a], alphas[a], sigmas[a]).run(env, n_iter) returns after
    torch.manual_seed(seeds[a]); np.random.seed(seeds[a]).  The global generators are not touched.

    After run(): weights [A, n, net_doubles(n)], state [A, d], status and actor_updates [A]."""

    def __init__(self, env, gammas, alphas, sigmas, seeds):
        self.env = env
        self.gammas, self.alphas, self.sigmas = (np.asarray(v, dtype=np.float64).reshape(-1)
                                                 for v in (gammas, alphas, sigmas))
        self.seeds = [int(s) for s in seeds]
        A = len(self.seeds)
        if A < 1 or not (len(self.gammas) == len(self.alphas) == len(self.sigmas) == A):
            raise ValueError("gammas, alphas, sigmas and seeds must have the same length, at least 1")
        self.n_agent = A
        self.weights = self.state = self.status = self.actor_updates = None

    def run(self, n_iter, chunk=2048, train=True):
        env = self.env
        weights, draw, state = draw_batch(env, self.seeds, self.sigmas)
        run = _Run(env._params(), env.device, self.gammas, self.alphas, weights, state)
        rewards = run.run(int(n_iter), int(chunk), bool(train), draw)
        self.weights = run.weights.cpu().numpy()
        self.state = run.state.cpu().numpy()
        self.status = run.status.cpu().numpy()
        self.actor_updates = run.actor_updates.cpu().numpy()
        return rewards


class CACLA_LQR_agent:
    """Drop-in for the reference's CACLA_LQR_agent (cacla_agent.py:202-297): CACLA on an LQR environment
    (envs.gym_lqr) with the linear actor F [n_ac, n_obs] and the quadratic critic V [n_obs], kept across runs.
    run() is the reference's loop on the fused kernel (sw_lqr_cacla_run_f64, cacla/lqr.py); the host forward and
    backward methods are the reference's, for evaluating a learnt agent by hand.

    After run(): admitted (steps taken; n_iter here), violations (0 here), actor_updates (steps with temp_diff > 0)
    and status (SW_STATUS_NONFINITE when F, V or the state overflowed); the environment's state is the run's last."""

    chunk = 2048       # steps per launch
    device = "cuda:0"

    def __init__(self, env):
        self.env = env
        n_obs = env.observation_space.shape[0]
        n_ac = env.action_space.shape[0]
        self.F = np.zeros((n_ac, n_obs))
        self.V = np.zeros(n_obs)
        self.admitted = self.violations = self.actor_updates = self.status = 0

    def forward_action_FA(self, state):
        """The linear actor: F s."""
        return self.F @ np.asarray(state, dtype=np.float64)

    def backward_action_FA(self, alpha, action, state, FA_action):
        """F_ij += (alpha (action_i - FA_action_i)) state_j."""
        step = alpha * (np.asarray(action, dtype=np.float64) - np.asarray(FA_action, dtype=np.float64))
        self.F += np.outer(step, np.asarray(state, dtype=np.float64))

    def forward_value_FA(self, state):
        """The quadratic critic: sum_j V_j s_j^2."""
        return self.V @ np.square(np.asarray(state, dtype=np.float64))

    def backward_value_FA(self, alpha, delta, state):
        """V_j += (alpha delta) s_j^2."""
        self.V += (alpha * delta) * np.square(np.asarray(state, dtype=np.float64))

    def run(self, n_iter, gamma, alpha, sigma, H=1000):
        """-> (states [n_iter, n_obs], actions [n_iter, n_ac], rewards [n_iter]), as the reference."""
        from . import lqr
        return lqr.run_single(self, "plain", n_iter, gamma, alpha, sigma, H)
