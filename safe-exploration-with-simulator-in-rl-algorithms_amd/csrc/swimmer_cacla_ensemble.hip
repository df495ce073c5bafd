// swimmer_cacla_ensemble.hip -- CACLA on the swimmer, every real step gated on an ENSEMBLE of up to 64 simulators, the
// members in the lanes of the agent's wave: sw_cacla_safe_ensemble_run_f64 and the seven cacla::gated_kernel<N, true>
// behind it.  The kernel, the argument check and the launch are swimmer_cacla_gated.h, shared with the gate in one
// simulator (swimmer_cacla_safe.hip); its header explains where the members live and the two optional records.  A
// translation unit of its own: no other code object depends on it.
#include "swimmer_cacla_gated.h"

int sw_cacla_safe_ensemble_run_f64(const sw_params *real, int64_t n_agent, int32_t n_member, int32_t n_iter,
                                   int64_t t_begin, const double *gamma, const double *alpha, const double *noise,
                                   const int32_t *gated, const double *sims, const double *sim_thresh,
                                   const double *real_thresh, int32_t cost_kind, int32_t cost_index, double *weights,
                                   double *state, double *last_reward, double *rewards, int32_t *admitted_rec,
                                   double *worst_rec, int32_t *member_refusals, int32_t *counters,
                                   int32_t *first_refused, int32_t *status, void *stream)
{
    const cacla::GatedArgs<true> a{gamma,   alpha,       noise,   gated,        sims,      sim_thresh,      real_thresh,
                                   weights, state,       last_reward, rewards,  admitted_rec, worst_rec,    member_refusals,
                                   counters, first_refused, status};
    return cacla::gated_run<true>(real, n_agent, n_member, n_iter, t_begin, cost_kind, cost_index, a, stream);
}
