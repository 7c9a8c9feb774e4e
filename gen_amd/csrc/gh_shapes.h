// gh_shapes.h — the instantiated model shapes, stated once (macros only, no
// includes): the state dimensions, the LG-SSM structures and slot variants of
// each, and how the dimensions are binned over the instantiating units.
//
// A feature header defines its kernel set GH_<F>_KERNELS(X, M, P) — X is
// `template` (the instantiating unit) or `extern template` (gh_api.hip), M the
// model type, P its parameter struct — and the shapes come from here:
//   GH_BIN_LIGHT_LG1(GH_LG_EACH, GH_FC_KERNELS, template)   one unit's share
//   GH_FOR_D(GH_LG_EACH, GH_FC_KERNELS, extern template)    every dimension
#pragma once

// F(..., 1) ... F(..., 16): the one place that enumerates the state dimensions
// (`...`: the arguments F takes before the dimension)
#define GH_FOR_D(F, ...)                                                                                      \
  F(__VA_ARGS__, 1) F(__VA_ARGS__, 2) F(__VA_ARGS__, 3) F(__VA_ARGS__, 4) F(__VA_ARGS__, 5) F(__VA_ARGS__, 6) \
  F(__VA_ARGS__, 7) F(__VA_ARGS__, 8) F(__VA_ARGS__, 9) F(__VA_ARGS__, 10) F(__VA_ARGS__, 11)                 \
  F(__VA_ARGS__, 12) F(__VA_ARGS__, 13) F(__VA_ARGS__, 14) F(__VA_ARGS__, 15) F(__VA_ARGS__, 16)

// the model types (a macro argument of their own, so their comma survives)
#define GH_LGM(D, S) gh::LGModel<D, S>
#define GH_SLM(D, L) gh::SlotModel<D, L>

// K over the shapes of dimension D: the four exact-zero structures of the
// LG-SSM; the plain and the extended (a library slot or the switching latent)
// slot model
#define GH_LG_EACH(K, X, D) \
  K(X, GH_LGM(D, 0), gh::LGParams) K(X, GH_LGM(D, 1), gh::LGParams) K(X, GH_LGM(D, 2), gh::LGParams) \
  K(X, GH_LGM(D, 3), gh::LGParams)
#define GH_SL_EACH(K, X, D) K(X, GH_SLM(D, false), gh::SlotParams) K(X, GH_SLM(D, true), gh::SlotParams)

// The dimensions of each instantiating unit gh_inst_<feature><k>.hip, balanced
// for build time (the kernels grow as d^2).  Each partition covers 1..16 once.
// heavy (lg, grad, slice):
#define GH_BIN_HEAVY0(F, ...) \
  F(__VA_ARGS__, 1) F(__VA_ARGS__, 2) F(__VA_ARGS__, 3) F(__VA_ARGS__, 4) F(__VA_ARGS__, 5) F(__VA_ARGS__, 6)
#define GH_BIN_HEAVY1(F, ...) F(__VA_ARGS__, 7) F(__VA_ARGS__, 8) F(__VA_ARGS__, 9)
#define GH_BIN_HEAVY2(F, ...) F(__VA_ARGS__, 10) F(__VA_ARGS__, 11)
#define GH_BIN_HEAVY3(F, ...) F(__VA_ARGS__, 12) F(__VA_ARGS__, 13)
#define GH_BIN_HEAVY4(F, ...) F(__VA_ARGS__, 14)
#define GH_BIN_HEAVY5(F, ...) F(__VA_ARGS__, 15)
#define GH_BIN_HEAVY6(F, ...) F(__VA_ARGS__, 16)
// slots (units 0..3 the plain models, 4..7 the extended ones over the same bins):
#define GH_BIN_SLOTS0(F, ...) \
  F(__VA_ARGS__, 1) F(__VA_ARGS__, 2) F(__VA_ARGS__, 3) F(__VA_ARGS__, 4) F(__VA_ARGS__, 5) F(__VA_ARGS__, 6)
#define GH_BIN_SLOTS1(F, ...) F(__VA_ARGS__, 7) F(__VA_ARGS__, 8) F(__VA_ARGS__, 9) F(__VA_ARGS__, 10)
#define GH_BIN_SLOTS2(F, ...) F(__VA_ARGS__, 11) F(__VA_ARGS__, 12) F(__VA_ARGS__, 13)
#define GH_BIN_SLOTS3(F, ...) F(__VA_ARGS__, 14) F(__VA_ARGS__, 15) F(__VA_ARGS__, 16)
// light (forecast, smooth, ancestor), the LG-SSM in units 0..3:
#define GH_BIN_LIGHT_LG0(F, ...)                                                                              \
  F(__VA_ARGS__, 1) F(__VA_ARGS__, 2) F(__VA_ARGS__, 3) F(__VA_ARGS__, 4) F(__VA_ARGS__, 5) F(__VA_ARGS__, 6) \
  F(__VA_ARGS__, 7)
#define GH_BIN_LIGHT_LG1(F, ...) F(__VA_ARGS__, 8) F(__VA_ARGS__, 9) F(__VA_ARGS__, 10) F(__VA_ARGS__, 11)
#define GH_BIN_LIGHT_LG2(F, ...) F(__VA_ARGS__, 12) F(__VA_ARGS__, 13) F(__VA_ARGS__, 14)
#define GH_BIN_LIGHT_LG3(F, ...) F(__VA_ARGS__, 15) F(__VA_ARGS__, 16)
// and the slot models in units 4..6:
#define GH_BIN_LIGHT_SL0(F, ...)                                                                              \
  F(__VA_ARGS__, 1) F(__VA_ARGS__, 2) F(__VA_ARGS__, 3) F(__VA_ARGS__, 4) F(__VA_ARGS__, 5) F(__VA_ARGS__, 6) \
  F(__VA_ARGS__, 7) F(__VA_ARGS__, 8)
#define GH_BIN_LIGHT_SL1(F, ...) F(__VA_ARGS__, 9) F(__VA_ARGS__, 10) F(__VA_ARGS__, 11) F(__VA_ARGS__, 12)
#define GH_BIN_LIGHT_SL2(F, ...) F(__VA_ARGS__, 13) F(__VA_ARGS__, 14) F(__VA_ARGS__, 15) F(__VA_ARGS__, 16)
