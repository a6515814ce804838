// pg_covariance.hpp -- what pg_covariance.hip needs from the pose-graph engine (pg_engine.hip); the host-side gauge check,
// pg_gauge_fixed, is pg_plan.hpp's.
#pragma once
#include <string>
#include <vector>

#include "common.hpp"
#include "pg_plan.hpp"

struct stba_pg;

namespace stba {

// the graph as the caller gave it (host copies kept by the engine) -- enough to refuse a request before any device work
struct PgCovGraph {
    int n = 0, m = 0;
    const int* ei = nullptr; const int* ej = nullptr;      // [m]
    const unsigned char* fixed = nullptr;                  // [n] or null
    bool several_ranks = false;                            // an all-reduce hook or communicator is set
    const unsigned char* anchored = nullptr;               // [n] or null: the node holds a pose prior and is not constant
};
void pg_cov_graph(const stba_pg* g, PgCovGraph* out);

// the linearisation at the engine's current poses, on the device.  pg_cov_linearize re-linearises and sums the diagonal blocks (the priors' included); it
// writes only buffers that every stba_pg_solve overwrites before it reads them (residuals, Jacobians, gradient, diagonal blocks).
struct PgCovDevice {
    hipStream_t st = nullptr;
    const int* node_start = nullptr;       // [n + 1]: the edge ends of every node (CSR)
    const int* end_code = nullptr;         // [2 m]: 2 * edge + side at a CSR position
    const int* end_rem = nullptr;          // [2 m]: the node at the other end
    const double* Ji = nullptr; const double* Jj = nullptr;      // [36][m] component-major, zero for constant nodes
    const double* Hd = nullptr;            // [n][36] diagonal blocks of J^T J
    const unsigned char* fixed = nullptr;  // device, or null
    // node pose priors (both null: none): the node's slot or -1 [n], and the slots' summed blocks J'^T J' [slots][36], which Hd holds too
    const int* node_slot = nullptr;
    const double* Hp = nullptr;
};
int pg_cov_linearize(stba_pg* g, PgCovDevice* out);

}  // namespace stba
