"""Augmented Random Search driver: mirror of the reference `ARSAgent`
(ars/ars_agent.py:16-220, the unsafe V1/V2 path).

Same constructor arguments, same public methods (runOneIteration, runTraining,
sort_directions, update_policy) and attributes (policy, mean, covariance, agent_param,
database), same random stream (NumPy's global legacy generator, seeded in __init__, deltas
drawn as 2*rand(m, d)-1, ars_agent.py:95,137).  What differs is where the work happens:

  * the N perturbations and the 2N rollouts of an iteration are ONE launch of the fused
    rollout kernel (sw_ars_rollouts_f64) on this rank's shard of the directions;
  * returns and V2 moment rows are exchanged with ONE all-gather (RCCL) per iteration;
  * sigma_R, the policy step and the running V2 statistics are ONE launch of
    sw_ars_update_f64, run redundantly and deterministically on every rank;
  * the full state covariance (only its diagonal feeds the policy, ars/environment.py:32)
    is one HBM-bound pass over the recorded trajectories (sw_traj_moments_f64) that rides
    along in the next iteration's rollout launch.  With more than one rank every rank holds
    the sums of its own shard: `reduce_covariance()` is the (explicit) collective that adds
    them up; the `covariance` attribute itself never communicates.

Safe exploration (agent_param.safe=True, ars_agent.py:40-66, :144-157): before any real rollout,
both rollouts P +- nu*delta_i of every direction run in a SIMULATOR built from the estimated
parameters, and the direction is admitted only if neither simulator return is <= sim_threshold.
Within an iteration the gate of direction i depends on the policy, delta_i, the frozen V2
statistics and the estimated parameters only, so the 2N simulator rollouts are ONE launch of
sw_ars_gate_f64 (returns only, the decision fused into the kernel).  The admit flags are the ONE
device->host read the safe path adds per iteration; the admitted deltas, packed in ascending
direction order, then go through the same pipeline as above with n_dir = k (k = admitted count),
and nothing is enqueued when k = 0.  Deviation where the reference has no answer: with N > 1 and
some but not all directions refused, the reference's sort_directions indexes rewards[2*i] for
every i < N and raises IndexError (ars_agent.py:105); here only the k admitted directions are
ranked and used, each with its own delta, sigma_R is taken over their 2k returns, the step is
divided by agent_param.b as in the reference, and top_b is clamped to k.  For N = 1, and for
iterations where all or none of the directions pass, this is the reference's behaviour.  Argument
errors the reference only meets later are raised at construction: sim_thresh=None and a missing
data_path raise ValueError; the gate is not sharded, so more than one rank raises
NotImplementedError.

The gate in an ENSEMBLE of simulators (sim_ensemble: a list of EnvParam, ars/ensemble.py): where the reference
leaves `# TODO compute sim_threshold` (ars_agent.py:70), the gate of an iteration is one sw_ars_gate_ensemble_f64
call -- every member's 2N rollouts, then the fold -- and a direction is admitted only where every member admits it.
sim_thresh may then be None: the simulator threshold is agent_param.threshold itself, the worst member standing where
alpha(H) * epsilon stood (a Threshold still adds its margin).  estimated_param is member 0; last_worst holds the worst
simulated returns [2N] of the last iteration, read in the same copy as the flags.  The rest of the iteration is the
safe iteration as it was.

Streams: every launch goes to torch's CURRENT stream.  With a NCCL process group alive, work on
the null (default) stream is implicitly ordered against the group's streams, which costs an
iteration ~13 us of device-side waits (measured); run distributed training under a stream of
its own, e.g. torch.cuda.set_stream(torch.cuda.Stream()), as bench.py does.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from .. import kernels
from .._lib import (SwParams, SwimmerHipError, kernel_flags, numpy_global_uniform_pm1,
                    require_gpu)
from .database import Database
from .ensemble import check_ensemble, sim_rows
from .ensemble_kernels import ars_gate_ensemble
from .environment import Environment
from . import sharding as _sh
from .sharding import (all_gather_segments, returns_from_segments, segment_len,
                       shard_bounds)


def approximate_env_param(env_param, approx_error):
    """The reference's approximation branch (ars_agent.py:45-53): a direction drawn from NumPy's
    global generator (rand(3), normalised) scaled by approx_error, added to m_i, l_i, k.  Like the
    reference it MUTATES and returns `env_param` itself (renamed 'LeonSwimmer-Simulator')."""
    unknowns = ('m_i', 'l_i', 'k')
    delta = np.random.rand(len(unknowns))
    delta = delta / np.linalg.norm(delta, ord=2) * approx_error
    env_param.name = 'LeonSwimmer-Simulator'
    env_param.m_i += delta[0]
    env_param.l_i += delta[1]
    env_param.k += delta[2]
    return env_param


def approximate_env_params(env_param, approx_error, count, rng=None):
    """`count` simulators for the agents of a batch (SafeARSAgentBatch): agent s gets the approximation branch above
    on ITS OWN copy of `env_param`, as each Ray actor of the reference's ars/safe_exploration.py does on the copy it
    was sent.  The draws are rand(3) each, taken in agent order from `rng` (a RandomState; default: NumPy's global
    generator), with the arithmetic of approximate_env_param, so agent 0 is what approximate_env_param gives under
    the same generator state.  `env_param` itself is not touched."""
    import copy
    rand = np.random.rand if rng is None else rng.rand
    out = []
    for _ in range(int(count)):
        sim = copy.copy(env_param)
        delta = rand(3)
        delta = delta / np.linalg.norm(delta, ord=2) * approx_error
        sim.name = 'LeonSwimmer-Simulator'
        sim.m_i += delta[0]
        sim.l_i += delta[1]
        sim.k += delta[2]
        out.append(sim)
    return out


def simulator_threshold(agent_param, real_env_param, sim_thresh):
    """threshold + alpha(H) * epsilon (ars_agent.py:59-63)."""
    alpha = sim_thresh.compute_alpha(agent_param.H)
    return agent_param.threshold + alpha * real_env_param.epsilon


class ARSAgent(object):

    def __init__(self, real_env_param, agent_param, data_path=None, seed=None,
                 guess_param=None, approx_error=None, sim_thresh=None, *, device=None,
                 process_group=None, record_trajectories=False, full_covariance=True,
                 top_b=0, rollout_kernel="auto", direct_rccl=None, estimator_options=None, sim_ensemble=None):
        self.safe = bool(agent_param.safe)
        if sim_ensemble is not None:
            # the gate in an ensemble of simulators (ars/ensemble.py): the members ARE the estimation
            if not self.safe:
                raise ValueError("sim_ensemble gates a safe agent: agent_param.safe must be True")
            if guess_param is not None or approx_error is not None:
                raise ValueError("sim_ensemble is the estimation: guess_param and approx_error must be None")
            sim_ensemble = check_ensemble(sim_ensemble, real_env_param)
        if self.safe:
            # the reference reaches `...` (ars_agent.py:64-65) / np.load(None) and fails later
            if sim_thresh is None and sim_ensemble is None:
                raise ValueError("safe=True needs sim_thresh (a Threshold) to set the simulator threshold")
            if data_path is None:
                raise ValueError("safe=True needs data_path: the real-world trajectories the agent loads")
        self.distributed = dist.is_available() and dist.is_initialized()
        self.group = process_group
        self.world = dist.get_world_size(process_group) if self.distributed else 1
        self.rank = dist.get_rank(process_group) if self.distributed else 0
        if self.safe and self.world > 1:
            raise NotImplementedError("safe=True runs on one rank: the simulator gate is not sharded")
        require_gpu()
        if device is None:
            device = f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}"
        self.device = torch.device(device)

        self.real_env_param = real_env_param
        self.real_world = Environment(real_env_param, device=device)
        self.agent_param = agent_param
        self.database = Database()
        self.record_trajectories = record_trajectories
        self.full_covariance = full_covariance and not agent_param.V1
        self.top_b = int(top_b)

        n = real_env_param.n
        self.m, self.d = n - 1, 2 * n + 2
        # direction / max_u keep the env defaults, as in the reference (environment.py:15-17)
        self.params = SwParams.make(n, real_env_param.l_i, real_env_param.m_i,
                                    real_env_param.k, real_env_param.h, (1.0, 0.0),
                                    flags=kernel_flags(rollout_kernel))
        # Safe exploration (ars_agent.py:40-66).  self.params above holds the real world's values
        # from BEFORE the approximation branch mutates real_env_param, as the reference's real_world
        # env was built before it.
        self.violations = 0                            # real returns below threshold so far
        self.last_admitted = np.zeros(0, dtype=np.int64)
        self.estimated_param = self.sim_threshold = self.p_sim = None
        self.sim_ensemble = sim_ensemble
        self.last_worst = np.zeros(0)                  # the ensemble gate's worst simulated returns, [2N]
        if self.safe:
            self.database.load(data_path)
            if sim_ensemble is not None:
                print(f"Using an ensemble of {len(sim_ensemble)} simulators...")
                self.estimated_param = sim_ensemble[0]
            elif guess_param is not None:
                from .estimator import Estimator    # CMA-ES: `cma` when it imports, else the built-in search
                print("Using computed estimation...")
                self.estimated_param = Estimator(self.database, guess_param,
                                                 capacity=1).estimate_real_env_param(**(estimator_options or {}))
            elif approx_error is not None:
                print("Using approximated estimation...")
                self.estimated_param = approximate_env_param(real_env_param, approx_error)
            else:
                print("Using exact estimation...")
                self.estimated_param = real_env_param
            print(f"Used estimation: {self.estimated_param}")
            # with an ensemble the worst member stands where alpha * epsilon stood: the safety threshold itself,
            # unless the caller still wants a margin on top
            self.sim_threshold = (agent_param.threshold if sim_thresh is None else
                                  simulator_threshold(agent_param, real_env_param, sim_thresh))
            print(f"Simulator threshold is {self.sim_threshold}")
            est = self.estimated_param
            self.p_sim = SwParams.make(est.n, est.l_i, est.m_i, est.k, est.h, (1.0, 0.0),
                                       flags=kernel_flags(rollout_kernel))
        if agent_param.initial_w == 'Zero':
            policy = np.zeros((self.m, self.d))
        else:
            policy = np.load(agent_param.initial_w)
            assert policy.shape == (self.m, self.d)

        f64 = dict(dtype=torch.float64, device=self.device)
        self._policy = torch.as_tensor(np.ascontiguousarray(policy, dtype=np.float64),
                                       device=self.device)
        self.v2 = not agent_param.V1
        self._mean = torch.zeros(self.d, **f64) if self.v2 else None
        self._inv_std = torch.ones(self.d, **f64) if self.v2 else None
        self._running = torch.zeros(1 + 2 * self.d, **f64) if self.v2 else None
        self._sigma = torch.zeros(1, **f64)
        self.n_saved_states = 0

        N, H = agent_param.N, agent_param.H
        self.lo, self.hi, self.chunk = shard_bounds(N, self.rank, self.world)
        self.n_local = self.hi - self.lo
        # covariance sums of this rank's shard [count | sum x | sum x x^T] + the pass's scratch
        self._cov_sums = 1 + self.d + self.d * self.d
        cov_doubles = kernels.cov_acc_doubles(self.params, 2 * self.n_local, H)
        if self.safe:
            # a safe iteration's pass covers the 2k admitted rollouts; the scratch a pass needs is
            # not monotone in the rollout count, so size it for every k <= N
            cov_doubles = max(kernels.cov_acc_doubles(self.params, 2 * k, H) for k in range(1, N + 1))
        self._cov_acc = (torch.zeros(cov_doubles, **f64) if self.full_covariance else None)
        self._coll_events = None
        self._cov_total = None       # all ranks' sums as of iteration _cov_total_it (world > 1)
        self._cov_total_it = -1
        self.rows_chunk = kernels.moments_blocks(2 * self.chunk) if self.v2 else 0
        # Ring-buffered pipeline (slot = iteration mod ring depth), enqueued from native code
        # (sw_ars_pipeline, include/swimmer_hip.h):
        #   copy stream : H2D of the deltas, overlaps the tail of the previous iteration
        #   main stream : rollouts -> all-gather -> update   (the critical path, kernels only);
        #                 the full-covariance pass over iteration i's trajectories rides along
        #                 in the rollout launch of iteration i + 1 (only diag(cov) feeds the
        #                 policy, and that comes from the moments fused into the rollout kernel)
        self._pipe = kernels.ArsPipeline()
        ring = self._pipe.slots
        self._deltas2 = [torch.empty((N, self.m, self.d), **f64) for _ in range(ring)]
        self._deltas = self._deltas2[0]
        self._deltas_host = [torch.empty((N, self.m, self.d), dtype=torch.float64).pin_memory()
                             for _ in range(ring)]
        self._deltas_host_np = [t.numpy() for t in self._deltas_host]
        self._it = 0
        # This rank's results live in ONE packed segment [2*chunk returns | moment rows]
        # (zero padded): the kernels write into views of it, the all-gather ships it as is,
        # and the update kernel indexes the gathered buffer in place.
        width = 2 * self.d
        self._seg_len = segment_len(self.chunk, self.rows_chunk, width)
        self._send = torch.zeros(self._seg_len, **f64)
        self._gathered = (torch.zeros(self.world * self._seg_len, **f64)
                          if (self.world > 1 or _sh._FORCE_COLLECTIVE) else self._send)
        self._returns_local = self._send[:2 * self.n_local]
        rows_local = kernels.moments_blocks(2 * self.n_local) if self.v2 else 0
        self._moments_local = (self._send[2 * self.chunk:2 * self.chunk + rows_local * width]
                               .view(rows_local, width) if self.v2 else None)
        need_traj = self.full_covariance or record_trajectories
        self._traj2 = ([torch.empty((H, self.d, 2 * self.n_local), **f64) for _ in range(ring)]
                       if need_traj and self.n_local > 0 else [None] * ring)
        self._traj = self._traj2[0]
        self._status = torch.zeros(max(1, 2 * self.n_local), dtype=torch.int32,
                                   device=self.device)
        if self.safe:
            self._gate_deltas = torch.empty((N, self.m, self.d), **f64)
            self._gate_returns = torch.empty(2 * N, **f64)
            # [admit (N) | simulator status (2N)]: read back with ONE device->host copy
            self._gate_flags = torch.zeros(3 * N, dtype=torch.int32, device=self.device)
            if sim_ensemble is not None:
                E = len(sim_ensemble)
                # [worst (2N doubles) | admit (N) | folded status (2N)] in ONE buffer: still one device->host copy
                self._gate_read = torch.zeros(16 * N + 12 * N, dtype=torch.uint8, device=self.device)
                self._gate_worst = self._gate_read[:16 * N].view(torch.float64).view(1, 2 * N)
                self._gate_flags = self._gate_read[16 * N:].view(torch.int32)
                self._ens_sim = torch.as_tensor(sim_rows(sim_ensemble)[None], device=self.device)
                self._ens_thresh = torch.full((1,), float(self.sim_threshold), **f64)
                self._ens_thresh_host = self.sim_threshold
                self._ens_returns = torch.empty((1, E, 2 * N), **f64)
                self._ens_status = torch.zeros((1, E, 2 * N), dtype=torch.int32, device=self.device)
                self._ens_admit = torch.zeros((1, E, N), dtype=torch.int32, device=self.device)

        # The exchange: torch.distributed (default), or -- direct_rccl=True / SWIMMER_DIRECT_RCCL=1 --
        # ncclAllGather called from native code on the critical stream with a communicator of this
        # agent's own (sw_comm, include/swimmer_hip.h).  Same bytes either way; torch stays the
        # default until the direct path has met more than one rank.
        if direct_rccl is None:
            direct_rccl = os.environ.get("SWIMMER_DIRECT_RCCL", "0") not in ("", "0")
        self._comm = None
        if direct_rccl and (self.world > 1 or _sh._FORCE_COLLECTIVE):
            if self.world > 1 and dist.get_backend(self.group) != "nccl":
                raise SwimmerHipError("direct_rccl needs GPU ranks (backend nccl), one per device")
            # the communicator binds to the CURRENT device: make it this agent's (a torchrun job that never
            # called torch.cuda.set_device would otherwise put every rank's communicator on GPU 0)
            with torch.cuda.device(self.device):
                self._comm = kernels.DirectComm(self.world, self.rank, self._broadcast_bytes, self._all_ranks_ok)

        # Randomness: the reference seeds NumPy's global generator (ars_agent.py:94-95)
        self.n_seed = seed
        np.random.seed(self.n_seed)

    def _broadcast_bytes(self, payload):
        """Rank 0's 128 id bytes to every rank of the group (COLLECTIVE)."""
        if self.world == 1:
            return payload
        t = torch.zeros(128, dtype=torch.uint8, device=self.device)
        if self.rank == 0:
            t.copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        dist.broadcast(t, src=src, group=self.group)
        return bytes(t.cpu().numpy().tobytes())

    def _all_ranks_ok(self, ok):
        """COLLECTIVE: True when `ok` holds on every rank of the group."""
        if self.world == 1:
            return bool(ok)
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=self.group)
        return bool(t.item())

    def _exchange(self):
        if self._comm is not None:
            return self._comm.all_gather(self._send, self._gathered)
        return all_gather_segments(self._send, self._gathered, self.world, self.group)

    # ---- attributes the reference exposes -------------------------------------------
    @property
    def policy(self):
        return self._policy.cpu().numpy()

    @policy.setter
    def policy(self, value):
        self._policy.copy_(torch.as_tensor(np.ascontiguousarray(value, dtype=np.float64)))

    @property
    def mean(self):
        return None if not self.v2 else self._mean.cpu().numpy()

    @property
    def covariance(self):
        """np.cov(all saved states) (ddof = 1, ars_agent.py:182).  The diagonal is the one
        the policy whitening uses; off-diagonals need full_covariance=True.

        Never communicates.  With one rank it is always current.  With several ranks the
        off-diagonal sums are spread over the ranks: call `reduce_covariance()` on EVERY rank
        (a collective) after the iteration whose value is wanted; reading the attribute at any
        other time raises instead of blocking in a collective the other ranks never enter."""
        if not self.v2:
            return None
        if self.n_saved_states == 0:
            return np.identity(self.d)
        if not self.full_covariance:
            return np.diag(self._inv_std.cpu().numpy() ** -2.0)
        if self.world == 1:
            self._pipe.sync_cov()
            return self._cov_matrix(self._cov_acc[:self._cov_sums].cpu().numpy())
        if self._cov_total_it != self._it:
            raise SwimmerHipError(
                "covariance: the off-diagonal sums live on all ranks; call reduce_covariance() "
                "on every rank after the iteration (collective) before reading the attribute")
        return self._cov_matrix(self._cov_total)

    def reduce_covariance(self):
        """COLLECTIVE: add up every rank's covariance sums (they are linear) and return the
        covariance matrix; `covariance` then returns the same matrix on every rank until
        the next iteration.  A no-op beyond the local flush with one rank."""
        if not (self.v2 and self.full_covariance) or self.n_saved_states == 0:
            return self.covariance
        self._pipe.sync_cov()
        acc = self._cov_acc[:self._cov_sums]
        if self.world > 1:
            acc = acc.cpu() if dist.get_backend(self.group) == "gloo" else acc.clone()
            dist.all_reduce(acc, group=self.group)
        self._cov_total = acc.cpu().numpy()
        self._cov_total_it = self._it
        return self._cov_matrix(self._cov_total)

    def _cov_matrix(self, acc):
        n, s1 = acc[0], acc[1:1 + self.d]
        s2 = acc[1 + self.d:].reshape(self.d, self.d)
        cov = (s2 - np.outer(s1, s1) / n) / (n - 1.0)
        # the diagonal is the one the policy uses: the V2 running statistics
        cov[np.diag_indices(self.d)] = self._inv_std.cpu().numpy() ** -2.0
        return cov

    # ---- measurement aid: device time of the per-iteration all-gather ------------------
    def collective_timing(self, on):
        """HIP events on the launch stream around every all-gather from now on (off: None).
        Each pair costs a few microseconds of pipeline bubbles: keep it out of timed loops."""
        self._coll_events = [] if on else None

    def collective_us(self):
        """Mean device time between the end of the rollout launch and the start of the update,
        i.e. the all-gather as the critical stream sees it; None without samples."""
        if not self._coll_events:
            return None
        torch.cuda.synchronize(self.device)
        return 1e3 * sum(a.elapsed_time(b) for a, b in self._coll_events) / len(self._coll_events)

    # ---- pieces of an iteration -----------------------------------------------------
    def sample_deltas(self):
        """N perturbations, uniform on (-1, 1): the reference's exact call sequence
        (N draws of rand(m, d) from the global generator consume the stream exactly like
        one rand(N, m, d))."""
        return 2 * np.random.rand(self.agent_param.N, self.m, self.d) - 1

    def sort_directions(self, deltas, rewards):
        """Directions sorted by max(r+, r-), best first (ars_agent.py:97-108)."""
        r = np.asarray(rewards, dtype=np.float64).reshape(-1, 2)
        return np.argsort(r.max(axis=1)).tolist()[::-1]

    def update_policy(self, deltas, rewards, order):
        """P += alpha / (b sigma_R) sum_{i in order} (r_i+ - r_i-) delta_i
        (ars_agent.py:110-130), on the GPU.  `order` selects the directions used."""
        order = list(order)
        d = kernels._lib.dev_f64(np.asarray(deltas, dtype=np.float64)[order], self.device)
        r = np.asarray(rewards, dtype=np.float64).reshape(-1, 2)[order].reshape(-1)
        r = kernels._lib.dev_f64(r, self.device)
        kernels.ars_update(self.params, r, d, self._policy, self.agent_param.alpha,
                           self.agent_param.b, 0, sigma_out=self._sigma)

    def run_iteration_async(self, deltas=None, want_returns=True):
        """One ARS iteration without synchronising the host; returns the [2N] returns as a
        device tensor (a view of the result segment, valid until the next iteration), or
        None with want_returns=False."""
        if self.safe:
            return self._run_safe_iteration(deltas, want_returns)
        ap = self.agent_param
        i = self._pipe.next_slot()               # the pipeline's own count, not self._it
        self._it += 1
        self._pipe.host_slot_wait(i)             # the slot's previous user is done with it
        if self.record_trajectories:
            # the policy the rollouts are about to run with (the update below overwrites it)
            self._policy_snapshot = self._policy.cpu().numpy()
        host = self._deltas_host_np[i]
        if deltas is None:      # the same draws as sample_deltas(), generated natively
            numpy_global_uniform_pm1(host)
        else:
            host[...] = deltas
        self._deltas, self._traj = self._deltas2[i], self._traj2[i]
        self._pipe.rollouts(i, self.params, ap.N, self.lo, self.n_local, ap.H,
                            self._deltas_host[i], self._deltas, self._policy, ap.nu,
                            self._mean, self._inv_std, self._returns_local, self._traj,
                            self._moments_local,
                            self._cov_acc if self._traj is not None else None, self._status)
        if self._coll_events is not None and (self.world > 1 or _sh._FORCE_COLLECTIVE):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            gathered = self._exchange()
            e1.record()
            self._coll_events.append((e0, e1))
        else:
            gathered = self._exchange()
        n_new = 2 * ap.N * ap.H
        self._pipe.update(i, self.params, ap.N, gathered, self.world, self.chunk,
                          self.rows_chunk, self._deltas, self._policy, ap.alpha, ap.b,
                          self.top_b, self._running, n_new, self._mean, self._inv_std,
                          self._sigma)
        if self.v2:
            self.n_saved_states += n_new
        if self.record_trajectories and self._traj is not None:
            self.database.add_device_batch(self._traj.clone(),
                                           self._rollout_policies(host.copy()))
        if not want_returns:
            return None
        return returns_from_segments(gathered, ap.N, self.world, self.chunk)

    def _run_safe_iteration(self, deltas=None, want_returns=True):
        """One safe iteration (ars_agent.py:137-184): the gate launch over all N directions, ONE
        device->host read of its admit flags and simulator status codes (a failed simulator rollout raises
        LinAlgError, as a failed real rollout does), then the pipeline's real rollouts and update over the
        k admitted directions (packed in ascending order; none enqueued when k = 0).  Returns the
        2k real returns as a device tensor (a view of the result segment), or None."""
        ap = self.agent_param
        N, H = ap.N, ap.H
        i = self._pipe.next_slot()
        self._it += 1
        self._pipe.host_slot_wait(i)
        host = self._deltas_host_np[i]
        if deltas is None:      # the same draws as sample_deltas()
            numpy_global_uniform_pm1(host)
        else:
            host[...] = deltas
        self._gate_deltas.copy_(self._deltas_host[i], non_blocking=True)
        if self.sim_ensemble is not None:
            # every member's gate and the fold over them: one call, and worst comes back with the flags
            if self._ens_thresh_host != self.sim_threshold:      # sim_threshold is a public attribute: follow it
                self._ens_thresh_host = self.sim_threshold
                self._ens_thresh.fill_(float(self.sim_threshold))
            ars_gate_ensemble(self.p_sim, H, self._policy[None], self._gate_deltas[None], ap.nu, self._ens_sim,
                              self._ens_thresh, None if self._mean is None else self._mean[None],
                              None if self._inv_std is None else self._inv_std[None],
                              admit=self._gate_flags[:N].view(1, N), worst=self._gate_worst,
                              status=self._gate_flags[N:].view(1, 2 * N), member_returns=self._ens_returns,
                              member_status=self._ens_status, member_admit=self._ens_admit)
            read = self._gate_read.cpu().numpy()             # the one added device->host read
            self.last_worst = read[:16 * N].view(np.float64).copy()
            flags = read[16 * N:].view(np.int32)
        else:
            kernels.ars_gate(self.p_sim, H, self._policy, self._gate_deltas, ap.nu, 0, N, self.sim_threshold,
                             self._mean, self._inv_std, returns=self._gate_returns,
                             status=self._gate_flags[N:], admit=self._gate_flags[:N])
            flags = self._gate_flags.cpu().numpy()           # the one added device->host read
        if np.any(flags[N:] != 0):
            # a failed simulator rollout returns NaN, and NaN would admit its direction unnoticed
            raise np.linalg.LinAlgError("Singular matrix / non-finite state in a simulator rollout of the gate")
        admitted = np.flatnonzero(flags[:N])
        k = len(admitted)
        self.last_admitted = admitted
        if k == 0:
            return self._send[:0] if want_returns else None
        if self.record_trajectories:
            self._policy_snapshot = self._policy.cpu().numpy()
        if k < N:
            host[:k] = host[admitted]
        n_roll, width = 2 * k, 2 * self.d
        self._deltas = self._deltas2[i]
        traj = self._traj2[i]
        if traj is not None:    # [H, d, 2k] at the start of the [H, d, 2N] buffer
            traj = traj.view(-1)[:H * self.d * n_roll].view(H, self.d, n_roll)
        self._traj = traj
        moments = None
        if self.v2:
            rows, base = kernels.moments_blocks(n_roll), 2 * self.chunk
            moments = self._send[base:base + rows * width].view(rows, width)
            # the update sums all rows_chunk rows of the segment: the unused ones must add nothing
            self._send[base + rows * width:base + self.rows_chunk * width].zero_()
        self._pipe.rollouts(i, self.params, k, 0, k, H, self._deltas_host[i], self._deltas,
                            self._policy, ap.nu, self._mean, self._inv_std, self._send[:n_roll],
                            traj, moments, self._cov_acc if traj is not None else None,
                            self._status[:n_roll])
        gathered = self._exchange()
        n_new = 2 * k * H
        self._pipe.update(i, self.params, k, gathered, self.world, self.chunk, self.rows_chunk,
                          self._deltas, self._policy, ap.alpha, ap.b, min(self.top_b, k),
                          self._running, n_new, self._mean, self._inv_std, self._sigma)
        if self.v2:
            self.n_saved_states += n_new
        if self.record_trajectories and traj is not None:
            P, nd = self._policy_snapshot, ap.nu * host[:k]
            pols = np.empty((n_roll, self.m, self.d))
            pols[0::2] = P + nd
            pols[1::2] = P - nd
            self.database.add_device_batch(traj.clone(), pols)
        if not want_returns:
            return None
        return returns_from_segments(gathered, k, self.world, self.chunk)

    def _rollout_policies(self, deltas):
        """Host copy of the 2*n_local perturbed policies of this rank's shard, in rollout
        order (what the reference stores next to each trajectory, ars_agent.py:172)."""
        P = self._policy_snapshot
        out = np.empty((2 * self.n_local, self.m, self.d))
        nd = self.agent_param.nu * np.asarray(deltas)[self.lo:self.hi]
        out[0::2] = P + nd
        out[1::2] = P - nd
        return out

    # ---- checkpoint / resume (the reference only saves the policy, ars_agent.py:218-219) ----
    CHECKPOINT_FORMAT = 2   # 2: running = {n, mean - c, M2};  1: raw sums {n, S1, S2} (converted)

    def save_checkpoint(self, path):
        """Everything needed to continue training bit for bit: policy, V2 running statistics,
        covariance sums (per rank when distributed), iteration count and NumPy's global generator
        state.  Plain arrays in an .npz (no pickle).  Collective when distributed; rank 0 writes.
        Policy, returns and V2 statistics continue bit for bit at any world size whose shards are
        aligned to the 16-rollout moment rows; the full covariance continues bit for bit when
        the world size is the one that saved the file (else equal up to summation order)."""
        torch.cuda.synchronize(self.device)
        kind, key, pos, has_gauss, cached = np.random.get_state()
        assert kind == "MT19937"
        cov = cov_ranks = None
        if self.full_covariance:
            self._pipe.sync_cov()
            cov = self._cov_acc[:self._cov_sums]
            if self.world > 1:
                # every rank's own sums are kept (cov_acc_ranks): restoring them rank by rank keeps
                # the summation order, so a resume at the same world size is bit-exact for the
                # covariance too; cov_acc (their total) serves a resume at another world size
                cov = cov.cpu() if dist.get_backend(self.group) == "gloo" else cov.clone()
                parts = [torch.empty_like(cov) for _ in range(self.world)]
                dist.all_gather(parts, cov, group=self.group)
                cov_ranks = torch.stack(parts).cpu().numpy()
                cov = cov_ranks[0].copy()
                for r in range(1, self.world):
                    cov += cov_ranks[r]
            else:
                cov = cov.cpu().numpy()
        if self.rank == 0:
            data = dict(policy=self.policy, n_saved_states=np.int64(self.n_saved_states),
                        iteration=np.int64(self._it), rng_key=key, rng_pos=np.int64(pos),
                        rng_has_gauss=np.int64(has_gauss), rng_cached=np.float64(cached),
                        v2=np.int64(self.v2), format=np.int64(self.CHECKPOINT_FORMAT))
            if self.v2:
                data.update(mean=self._mean.cpu().numpy(), inv_std=self._inv_std.cpu().numpy(),
                            running=self._running.cpu().numpy())
            if cov is not None:
                data["cov_acc"] = cov
            if cov_ranks is not None:
                data["cov_acc_ranks"] = cov_ranks
            with open(path, "wb") as f:
                np.savez(f, **data)

    def load_checkpoint(self, path):
        z = np.load(path, allow_pickle=False)
        if bool(z["v2"]) != self.v2 or z["policy"].shape != (self.m, self.d):
            raise SwimmerHipError("checkpoint does not match this agent's configuration")
        # nothing of this agent's earlier iterations may still be in flight: the buffers below
        # are read by queued kernels (the update of the last iteration, an owed covariance pass)
        if self.full_covariance:
            self._pipe.sync_cov()
        torch.cuda.synchronize(self.device)
        dev = self.device
        self._policy.copy_(torch.as_tensor(z["policy"], device=dev))
        if self.v2:
            running = np.array(z["running"], dtype=np.float64)
            if "format" not in z.files or int(z["format"]) < 2:
                # round-1 files hold raw sums about the pivot: {n, S1, S2} -> {n, S1/n, S2 - S1^2/n}
                n, s1, s2 = running[0], running[1:1 + self.d], running[1 + self.d:]
                if n > 0:
                    running = np.concatenate(([n], s1 / n, s2 - s1 * (s1 / n)))
            self._mean.copy_(torch.as_tensor(z["mean"], device=dev))
            self._inv_std.copy_(torch.as_tensor(z["inv_std"], device=dev))
            self._running.copy_(torch.as_tensor(running, device=dev))
        if self.full_covariance:
            self._cov_acc.zero_()
            if "cov_acc_ranks" in z.files and z["cov_acc_ranks"].shape[0] == self.world:
                # same world size as the run that saved it: every rank takes its own sums back
                self._cov_acc[:self._cov_sums].copy_(torch.as_tensor(z["cov_acc_ranks"][self.rank], device=dev))
            elif "cov_acc" in z.files and self.rank == 0:
                # another world size (or a one-rank file): the total goes to rank 0 -- the sums are
                # linear, so the covariance is the same up to the order of the additions
                self._cov_acc[:self._cov_sums].copy_(torch.as_tensor(z["cov_acc"], device=dev))
        self._cov_total_it = -1
        self.n_saved_states = int(z["n_saved_states"])
        self._it = int(z["iteration"])
        np.random.set_state(("MT19937", z["rng_key"], int(z["rng_pos"]), int(z["rng_has_gauss"]),
                             float(z["rng_cached"])))
        torch.cuda.synchronize(self.device)

    def runOneIteration(self):
        """One whole ARS iteration (ars_agent.py:132-185); returns the list of 2N returns
        (safe=True: the 2k returns of the admitted directions' real rollouts, in order)."""
        rets = self.run_iteration_async()
        out = rets.cpu().numpy()
        status = self._status[:out.size] if self.safe else self._status
        if int((status != 0).sum().item()):
            raise np.linalg.LinAlgError("Singular matrix / non-finite state in a rollout")
        if self.safe:
            threshold = self.agent_param.threshold
            for reward in out:
                if reward < threshold:
                    print(f"Obtained in real world rollout a return of {reward}, below the "
                          f"threshold {threshold}")
                    self.violations += 1
        return out.tolist()

    def runTraining(self, save_data_path=None, save_policy_path=None):
        """1 warm-up iteration + n_iter iterations; curve = mean of the 2N returns
        (ars_agent.py:187-220)."""
        rewards = [np.mean(self.runOneIteration())]
        for j in range(1, self.agent_param.n_iter + 1):
            all_rewards = self.runOneIteration()
            r = np.mean(all_rewards) if len(all_rewards) > 0 else rewards[-1]
            rewards.append(r)
            if j % 10 == 0:
                if self.rank == 0:
                    ap, ep = self.agent_param, self.real_env_param
                    variant = "V1" if ap.V1 else "V2"
                    print(f"[seed {self.n_seed}] ARS {variant} n={ep.n} N={ap.N} b={ap.b} "
                          f"alpha={ap.alpha} nu={ap.nu} h={ep.h} l_i={ep.l_i} m_i={ep.m_i} | "
                          f"iteration {j}/{ap.n_iter}: mean return {r}")
                if save_data_path is not None:
                    # one rank: the reference's single file; several ranks: every rank stores the
                    # rollouts of its own shard (Database.shard_path / Database.load reads them all)
                    self.database.save(save_data_path, rank=self.rank, world=self.world)
        self.real_world.close()
        if save_policy_path is not None and self.rank == 0:
            np.save(save_policy_path, self.policy)
        return np.array(rewards)
