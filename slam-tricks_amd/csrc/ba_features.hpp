// ba_features.hpp -- which features of the bundle-adjustment engine go together: the tables of every refusal (DESIGN.md 7l prints them
// as one matrix; why there are two: see BA_REFUSALS_MORE).  A row says: the C function `asker`, called to SET its feature on an engine that holds `held`, returns `code` and
// leaves "<asker>: <text>" in stba_last_error().  Everything not in the table is supported.
// Host only: the standard library and include/stba.h, nothing of HIP, so that a plain C++ compiler builds it and
// tests/test_ba_factor_input_cpu.py checks it without a device (tests/cpp/ba_factor_input_driver.cpp).
#pragma once
#include <string>

#include "../../include/stba.h"

namespace stba {

enum BaFeature : unsigned {
    ITERATIVE_SCHUR = 1u << 0,      // fixed at creation (stba_ba_create_ex): it is held, never asked for
    DOGLEG = 1u << 1,               // stba_ba_set_trust_region
    INNER_ITERATIONS = 1u << 2,     // stba_ba_set_inner_iterations
    HOST_LINEARIZER = 1u << 3,      // stba_ba_set_host_linearizer
    // ONE bit for "an all-reduce hook" and "several ranks": stba_ba_set_allreduce refuses world_size > 1 without a hook, so on an
    // engine `ar || world > 1` and `ar` are the same condition
    ALLREDUCE = 1u << 4,
    LOSS = 1u << 5,                 // stba_ba_set_loss
    INFORMATION = 1u << 6,          // stba_ba_set_information / _sqrt_information
    POSE_PRIORS = 1u << 7,          // stba_ba_set_pose_priors
    RELATIVE_POSES = 1u << 8,       // stba_ba_set_relative_poses
    // behind the nine features BA_FEATURE_COUNT counts (see BA_REFUSALS_MORE below)
    LANDMARK_PRIORS = 1u << 9       // stba_ba_set_landmark_priors
};
constexpr int BA_FEATURE_COUNT = 9;
constexpr int BA_FEATURE_COUNT_ALL = 10;

// the features an engine holds, from plain values (the engine passes its members; a test passes what it likes)
inline unsigned ba_held_features(bool iterative, bool dogleg, bool inner_on, bool host_linearizer, bool allreduce, bool loss,
                                 bool information, int n_priors, int n_relative_poses, int n_landmark_priors = 0) {
    return (iterative ? ITERATIVE_SCHUR : 0u) | (dogleg ? DOGLEG : 0u) | (inner_on ? INNER_ITERATIONS : 0u) |
           (host_linearizer ? HOST_LINEARIZER : 0u) | (allreduce ? ALLREDUCE : 0u) | (loss ? LOSS : 0u) |
           (information ? INFORMATION : 0u) | (n_priors ? POSE_PRIORS : 0u) | (n_relative_poses ? RELATIVE_POSES : 0u) |
           (n_landmark_priors ? LANDMARK_PRIORS : 0u);
}

struct BaRefusal {
    const char* asker;
    unsigned held;          // the row applies when every bit of it is held (one feature, but for stba_ba_solve)
    int code;
    const char* text;
    bool when_clearing = false;     // the row applies to a call that CLEARS the asker's feature too
};

// The rows of one asker stand in the order the checks had when every function carried its own: with several conflicting features held,
// the first row names the reason.  The texts are kept byte for byte, irregular as they are: include/stba/ceres.h, g2o.h and the shim
// tests match on their words.  Three things are as they are on purpose (making them symmetric is another change):
//   * stba_ba_set_allreduce refuses an ITERATIVE_SCHUR or a DOGLEG engine even when the call clears the hook (when_clearing); its
//     other rows apply only when a hook is being set.
//   * DOGLEG with inner iterations is refused by stba_ba_solve, by neither setter: the row asks for BOTH features held.
//   * no row of a factor setter (loss, information, priors, relative poses) has when_clearing: a clearing call -- kind == NULL,
//     n == 0, in == NULL or all-identity weights -- is never refused.
#define STBA_INV STBA_ERR_INVALID_ARGUMENT
inline constexpr BaRefusal BA_REFUSALS[] = {
    {"stba_ba_set_host_linearizer", INNER_ITERATIONS, STBA_INV, "this engine has inner iterations (device residuals only)"},
    {"stba_ba_set_host_linearizer", LOSS, STBA_INV, "this engine has a loss table (losses need device residuals; not supported together)"},
    {"stba_ba_set_host_linearizer", INFORMATION, STBA_INV, "this engine has information matrices (the callback's factors whiten themselves; not supported together)"},
    {"stba_ba_set_host_linearizer", POSE_PRIORS, STBA_INV, "this engine has pose priors (priors need device residuals; not supported together)"},
    {"stba_ba_set_host_linearizer", RELATIVE_POSES, STBA_INV, "this engine has relative-pose factors (the factors need device residuals; not supported together)"},
    {"stba_ba_set_loss", HOST_LINEARIZER, STBA_INV, "this engine has a host lineariser (losses need device residuals; not supported together)"},
    {"stba_ba_set_loss", INNER_ITERATIONS, STBA_INV, "this engine has inner iterations (inner iterations with losses are not supported)"},
    {"stba_ba_set_loss", ALLREDUCE, STBA_INV, "this engine has an all-reduce hook, and losses run on one rank only"},
    {"stba_ba_set_information", HOST_LINEARIZER, STBA_INV, "this engine has a host lineariser (the callback's factors whiten themselves; not supported together)"},
    {"stba_ba_set_information", INNER_ITERATIONS, STBA_INV, "this engine has inner iterations (inner iterations with information matrices are not supported)"},
    {"stba_ba_set_information", ALLREDUCE, STBA_INV, "this engine has an all-reduce hook, and information matrices run on one rank only"},
    {"stba_ba_set_sqrt_information", HOST_LINEARIZER, STBA_INV, "this engine has a host lineariser (the callback's factors whiten themselves; not supported together)"},
    {"stba_ba_set_sqrt_information", INNER_ITERATIONS, STBA_INV, "this engine has inner iterations (inner iterations with information matrices are not supported)"},
    {"stba_ba_set_sqrt_information", ALLREDUCE, STBA_INV, "this engine has an all-reduce hook, and information matrices run on one rank only"},
    {"stba_ba_set_pose_priors", ITERATIVE_SCHUR, STBA_INV, "this engine uses ITERATIVE_SCHUR (its inexact-step model is summed from the observation records; pose priors are not supported)"},
    {"stba_ba_set_pose_priors", DOGLEG, STBA_INV, "this engine uses DOGLEG (DOGLEG with pose priors is not supported)"},
    {"stba_ba_set_pose_priors", INNER_ITERATIONS, STBA_INV, "this engine has inner iterations (inner iterations with pose priors are not supported)"},
    {"stba_ba_set_pose_priors", HOST_LINEARIZER, STBA_INV, "this engine has a host lineariser (priors need device residuals; not supported together)"},
    {"stba_ba_set_pose_priors", ALLREDUCE, STBA_INV, "this engine has an all-reduce hook, and pose priors run on one rank only"},
    {"stba_ba_set_relative_poses", ITERATIVE_SCHUR, STBA_INV, "this engine uses ITERATIVE_SCHUR (its inexact-step model is summed from the observation records; relative-pose factors are not supported)"},
    {"stba_ba_set_relative_poses", DOGLEG, STBA_INV, "this engine uses DOGLEG (DOGLEG with relative-pose factors is not supported)"},
    {"stba_ba_set_relative_poses", INNER_ITERATIONS, STBA_INV, "this engine has inner iterations (inner iterations with relative-pose factors are not supported)"},
    {"stba_ba_set_relative_poses", HOST_LINEARIZER, STBA_INV, "this engine has a host lineariser (the factors need device residuals; not supported together)"},
    {"stba_ba_set_relative_poses", ALLREDUCE, STBA_INV, "this engine has an all-reduce hook, and relative-pose factors run on one rank only"},
    {"stba_ba_set_allreduce", ITERATIVE_SCHUR, STBA_INV, "this engine uses ITERATIVE_SCHUR, which runs on one rank only", true},
    {"stba_ba_set_allreduce", DOGLEG, STBA_INV, "this engine uses DOGLEG, which runs on one rank only", true},
    {"stba_ba_set_allreduce", INNER_ITERATIONS, STBA_INV, "this engine has inner iterations, which run on one rank only"},
    {"stba_ba_set_allreduce", LOSS, STBA_INV, "this engine has a loss table, and losses run on one rank only"},
    {"stba_ba_set_allreduce", INFORMATION, STBA_INV, "this engine has information matrices, which run on one rank only"},
    {"stba_ba_set_allreduce", POSE_PRIORS, STBA_INV, "this engine has pose priors, which run on one rank only"},
    {"stba_ba_set_allreduce", RELATIVE_POSES, STBA_INV, "this engine has relative-pose factors, which run on one rank only"},
    {"stba_ba_set_trust_region", ITERATIVE_SCHUR, STBA_INV, "DOGLEG only supports exact factorization based linear solvers (this engine uses ITERATIVE_SCHUR)"},
    {"stba_ba_set_trust_region", ALLREDUCE, STBA_INV, "DOGLEG runs on one rank only (an all-reduce hook is set)"},
    {"stba_ba_set_trust_region", POSE_PRIORS, STBA_INV, "this engine has pose priors (DOGLEG with pose priors is not supported)"},
    {"stba_ba_set_trust_region", RELATIVE_POSES, STBA_INV, "this engine has relative-pose factors (DOGLEG with relative-pose factors is not supported)"},
    {"stba_ba_set_inner_iterations", ALLREDUCE, STBA_INV, "inner iterations run on one rank only (an all-reduce hook is set)"},
    {"stba_ba_set_inner_iterations", HOST_LINEARIZER, STBA_INV, "not with a host lineariser"},
    {"stba_ba_set_inner_iterations", LOSS, STBA_INV, "this engine has a loss table (inner iterations with losses are not supported)"},
    {"stba_ba_set_inner_iterations", INFORMATION, STBA_INV, "this engine has information matrices (inner iterations with information matrices are not supported)"},
    {"stba_ba_set_inner_iterations", POSE_PRIORS, STBA_INV, "this engine has pose priors (inner iterations with pose priors are not supported)"},
    {"stba_ba_set_inner_iterations", RELATIVE_POSES, STBA_INV, "this engine has relative-pose factors (inner iterations with relative-pose factors are not supported)"},
    {"stba_ba_inner_sweep", ALLREDUCE, STBA_INV, "one rank, device residuals only"},
    {"stba_ba_inner_sweep", HOST_LINEARIZER, STBA_INV, "one rank, device residuals only"},
    {"stba_ba_inner_sweep", LOSS, STBA_INV, "this engine has a loss table (inner iterations with losses are not supported)"},
    {"stba_ba_inner_sweep", INFORMATION, STBA_INV, "this engine has information matrices (inner iterations with information matrices are not supported)"},
    {"stba_ba_inner_sweep", POSE_PRIORS, STBA_INV, "this engine has pose priors (inner iterations with pose priors are not supported)"},
    {"stba_ba_inner_sweep", RELATIVE_POSES, STBA_INV, "this engine has relative-pose factors (inner iterations with relative-pose factors are not supported)"},
    {"stba_ba_solve", DOGLEG | INNER_ITERATIONS, STBA_INV, "inner iterations are not supported with DOGLEG"},
};

// The SECOND table: the rows of features that came after the first was pinned.  BA_REFUSALS, BA_FEATURE_COUNT and the answers for
// every mask of the first nine bits are held row for row by tests/golden/ba_refusals.json, so a later feature brings its rows here
// and gets a bit above them; ba_conflict searches this table behind the first (no asker has rows in both that could both apply to
// a mask of the first nine bits: every row here asks for a bit above them, or belongs to an asker the first table does not know).
// Landmark priors are block-diagonal in the landmark and go with ITERATIVE_SCHUR, DOGLEG, losses, weights, pose
// priors and relative poses; what they do not go with solves from, or sums over, the observation records alone.
inline constexpr BaRefusal BA_REFUSALS_MORE[] = {
    {"stba_ba_set_landmark_priors", INNER_ITERATIONS, STBA_INV, "this engine has inner iterations (the per-landmark sweep solves from the observation records; landmark priors are not supported)"},
    {"stba_ba_set_landmark_priors", HOST_LINEARIZER, STBA_INV, "this engine has a host lineariser (priors need device residuals; not supported together)"},
    {"stba_ba_set_landmark_priors", ALLREDUCE, STBA_INV, "this engine has an all-reduce hook, and landmark priors run on one rank only"},
    {"stba_ba_set_inner_iterations", LANDMARK_PRIORS, STBA_INV, "this engine has landmark priors (inner iterations with landmark priors are not supported)"},
    {"stba_ba_inner_sweep", LANDMARK_PRIORS, STBA_INV, "this engine has landmark priors (inner iterations with landmark priors are not supported)"},
    {"stba_ba_set_host_linearizer", LANDMARK_PRIORS, STBA_INV, "this engine has landmark priors (priors need device residuals; not supported together)"},
    {"stba_ba_set_allreduce", LANDMARK_PRIORS, STBA_INV, "this engine has landmark priors, which run on one rank only"},
};
#undef STBA_INV

// the first row of `asker` that an engine holding `held` meets: its code, and "<asker>: <text>" in *why; 0 if none.  `sets` is false
// for a call that clears the asker's feature (only the when_clearing rows apply)
inline int ba_conflict(const char* asker, unsigned held, std::string* why, bool sets = true) {
    const std::string who(asker);
    const auto applies = [&](const BaRefusal& r) { return who == r.asker && (held & r.held) == r.held && (sets || r.when_clearing); };
    for (const BaRefusal& r : BA_REFUSALS)
        if (applies(r)) { if (why) *why = who + ": " + r.text; return r.code; }
    for (const BaRefusal& r : BA_REFUSALS_MORE)
        if (applies(r)) { if (why) *why = who + ": " + r.text; return r.code; }
    return 0;
}

}  // namespace stba
