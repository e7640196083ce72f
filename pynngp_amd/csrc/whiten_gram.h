// Whitening of several columns by a stored NNGP factor and the Gram matrix of the result (whiten_gram.hip):
//   U = F^-1/2 (I - B) V,   G = U^T U
// the one small matrix the response-model regression (pynngp_amd/regression.py) is built on.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nngp {

constexpr int kWhitenMaxCols = 16;    // NNGP_WHITEN_MAX_COLS
constexpr int kGramChunkRows = 256;   // rows of U staged in LDS at a time
constexpr int kGramTileRows = 1024;   // rows per Gram record (one block): four chunks

struct WhitenArgs {
    const int32_t* nbr;    // (n_rows, m), row t
    const int32_t* order;  // null, or row t is local row order[t]
    const double* B;       // (n_rows, m), natural rows
    const double* F;       // (n_rows,), natural rows
    int64_t n_rows;
    int m;
    int64_t i0;
    int64_t n_points;
    int ncol;
    const double* V;   // (n_points, ncol)
    const double* Vq;  // null (S = T: the row's own values are V[i0 + row]) or (n_rows, ncol)
};

// records of the Gram fold: one per tile of kGramTileRows rows, ncol (ncol + 1) / 2 doubles each
int64_t whiten_gram_tiles(int64_t n_rows);
size_t whiten_gram_workspace_bytes(int64_t n_rows, int ncol);
// U (n_rows, ncol); gram null (whiten only) or (ncol, ncol).  n_rows = 0: no launch, gram zeroed.
hipError_t whiten_gram_launch(const WhitenArgs& a, double* U, double* gram, void* workspace, hipStream_t s);

}  // namespace nngp
