// gh_inst.h — the per-model kernels of the LG-SSM and slot families, for every
// shape of gh_shapes.h, are explicitly instantiated in the gh_inst_*.hip units
// (each one bin of dimensions) and only declared (extern template) in
// gh_api.hip, so the library's kernels compile in parallel translation units.
// The kernels' host stubs are ordinary external symbols: a launch in
// gh_api.hip finds the code object registered by the instantiating unit.
#pragma once
#include "gh_kernels.h"
#include "gh_rejuv.h"
#include "gh_scores.h"
#include "gh_simulate.h"
#include "gh_csmc.h"
#include "gh_slots.h"
#include "gh_grad.h"
#include "gh_slice.h"
#include "gh_shapes.h"

// X is `extern template` (declaration) or `template` (definition)
// the step kernel of a proposal's functor: init, plain, and the block remap
#define GH_STEP_KERNELS(X, M, P)                                                          \
  X __global__ void gh::k_step<M, true>(const double*, P, gh::StepObs, gh::StepArgs);     \
  X __global__ void gh::k_step<M, false>(const double*, P, gh::StepObs, gh::StepArgs);    \
  X __global__ void gh::k_step<M, false, true>(const double*, P, gh::StepObs, gh::StepArgs);
// every kernel of a model (the steps are spelled again: an M with a comma in
// it cannot be handed on to another macro).  `...`: what a unit lists after
// the model's first kernel: the slot units keep the linear proposal's steps
// there, so that their device code is unchanged.
#define GH_MODEL_KERNELS(X, M, P, ...)                                                                         \
  X __global__ void gh::k_step<M, true>(const double*, P, gh::StepObs, gh::StepArgs);                          \
  __VA_ARGS__                                                                                                  \
  X __global__ void gh::k_step<M, false>(const double*, P, gh::StepObs, gh::StepArgs);                         \
  X __global__ void gh::k_step<M, false, true>(const double*, P, gh::StepObs, gh::StepArgs);                   \
  X __global__ void gh::k_rejuv<M, true>(const double*, P, gh::StepObs, gh::RejuvArgs);                        \
  X __global__ void gh::k_rejuv<M, false>(const double*, P, gh::StepObs, gh::RejuvArgs);                       \
  X __global__ void gh::k_mh_drift<M, true>(const double*, P, gh::StepObs, gh::RejuvArgs, gh::DriftSd);        \
  X __global__ void gh::k_mh_drift<M, false>(const double*, P, gh::StepObs, gh::RejuvArgs, gh::DriftSd);       \
  X __global__ void gh::k_scores<M>(const double*, P, gh::ScoreArgs, const gh::DevScalars*);                   \
  X __global__ void gh::k_simulate<M>(const double*, P, gh::SimArgs);                                          \
  X __global__ void gh::k_mr_slot_scores<M>(const double*, P, gh::StepObs, int, const double*, const double*,  \
                                            const int32_t*, const double*, int64_t, int64_t, int64_t, double*, \
                                            int*);                                                             \
  X __global__ void gh::k_pin_pre<M, true>(const double*, P, gh::StepObs, gh::PinArgs);                        \
  X __global__ void gh::k_pin_pre<M, false>(const double*, P, gh::StepObs, gh::PinArgs);

// the LG-SSM of dimension D (gh_inst_lg<k>.hip, the heavy bins): its four
// structures, then the optimal and the linear proposal's step
#define GH_LG_DIM(X, D)                                 \
  GH_LG_EACH(GH_MODEL_KERNELS, X, D)                    \
  GH_STEP_KERNELS(X, gh::LGOptModel<D>, gh::LGParams)   \
  GH_STEP_KERNELS(X, gh::LGLinModel<D>, gh::LGParams)

// the slot family (gh_slots.h) of dimension D with the linear proposal's step:
// the plain models in gh_inst_slots0..3.hip, the extended in gh_inst_slots4..7.hip
#define GH_SL_LINM(D, L) gh::SlotLinModel<D, L>
#define GH_SL_KERNELS(X, D, L)                                    \
  GH_MODEL_KERNELS(X, GH_SLM(D, L), gh::SlotParams,               \
                   GH_STEP_KERNELS(X, GH_SL_LINM(D, L), gh::SlotParams))
#define GH_SL_PLAIN(X, D) GH_SL_KERNELS(X, D, false)
#define GH_SL_EXT(X, D) GH_SL_KERNELS(X, D, true)

// the gradient kernels (gh_grad.h): choice_gradients, mala and hmc for the
// continuous hand-lowered families, in gh_inst_grad<k>.hip
#define GH_GRAD_KERNELS(X, M, P)                                                                                  \
  X __global__ void gh::k_choice_gradients<M, true>(const double*, P, gh::StepObs, gh::RejuvArgs, double*);       \
  X __global__ void gh::k_choice_gradients<M, false>(const double*, P, gh::StepObs, gh::RejuvArgs, double*);      \
  X __global__ void gh::k_mala<M, true>(const double*, P, gh::StepObs, gh::RejuvArgs, double, double);            \
  X __global__ void gh::k_mala<M, false>(const double*, P, gh::StepObs, gh::RejuvArgs, double, double);           \
  X __global__ void gh::k_hmc<M, true>(const double*, P, gh::StepObs, gh::RejuvArgs, int, double);                \
  X __global__ void gh::k_hmc<M, false>(const double*, P, gh::StepObs, gh::RejuvArgs, int, double);

// the slice and map_optimize kernels (gh_slice.h) for the same families, in
// gh_inst_slice<k>.hip
#define GH_SLICE_KERNELS(X, M, P)                                                                                 \
  X __global__ void gh::k_elliptical_slice<M, true>(const double*, P, gh::StepObs, gh::RejuvArgs,                 \
                                                    unsigned long long*);                                         \
  X __global__ void gh::k_elliptical_slice<M, false>(const double*, P, gh::StepObs, gh::RejuvArgs,                \
                                                     unsigned long long*);                                        \
  X __global__ void gh::k_map_optimize<M, true>(const double*, P, gh::StepObs, gh::RejuvArgs, double, double,     \
                                                double);                                                          \
  X __global__ void gh::k_map_optimize<M, false>(const double*, P, gh::StepObs, gh::RejuvArgs, double, double,    \
                                                 double);
