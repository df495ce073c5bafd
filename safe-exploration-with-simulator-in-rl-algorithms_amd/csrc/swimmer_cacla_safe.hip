// swimmer_cacla_safe.hip -- CACLA on the swimmer WITH SAFE EXPLORATION, every real step gated by a one-step look-ahead
// in the agent's simulator: sw_cacla_safe_run_f64 and the seven cacla::gated_kernel<N, false> behind it.  The kernel,
// the argument check and the launch are swimmer_cacla_gated.h, shared with the ensemble gate
// (swimmer_cacla_ensemble.hip); its header explains the step, where the simulator lives and what an ungated agent
// computes.  A translation unit of its own: no other code object depends on it.
#include "swimmer_cacla_gated.h"

int sw_cacla_safe_run_f64(const sw_params *real, int64_t n_agent, int32_t n_iter, int64_t t_begin,
                          const double *gamma, const double *alpha, const double *noise, const int32_t *gated,
                          const double *sim, const double *sim_thresh, const double *real_thresh, int32_t cost_kind,
                          int32_t cost_index, double *weights, double *state, double *last_reward, double *rewards,
                          int32_t *admitted_rec, int32_t *counters, int32_t *first_refused, int32_t *status,
                          void *stream)
{
    const cacla::GatedArgs<false> a{gamma,   alpha,       noise,   gated,        sim,      sim_thresh,    real_thresh, weights,
                                    state,   last_reward, rewards, admitted_rec, counters, first_refused, status};
    return cacla::gated_run<false>(real, n_agent, 1, n_iter, t_begin, cost_kind, cost_index, a, stream);
}
