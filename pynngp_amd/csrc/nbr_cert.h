// Neighbour-set certificates (include/nngp.h nngp_nbr_cert_*): what a sweep may take for granted about a
// neighbour set that does not change between sweeps (a theta scan, an MCMC chain: coords, nbr and order live as
// long as the model; only theta and the values move).
//
// The pair kernel (bf_pairb.h) re-derives two facts per slot and sweep: that a neighbour index is in
// [0, n_points) (else the slot is a far-away padding point with a zero value), and that a squared distance is
// below the clamp d2max (nngp_math.h nngp_cov_unit).  The certificate settles both once:
//   * one bit per tile of pairb_tiling: CHECKED when any slot of any of the tile's rows is < 0 or >= n_points
//     (-1 padding and bad indices alike), else 0 = trusted;
//   * d2_span = sum over the dimensions of (max - min)^2 of the coordinates: no two points are farther apart,
//     so a sweep whose d2max exceeds it (one host compare per sweep, cert_trusted_tiles) never clamps a pair of
//     real points.
// Everything here compiles on the host alone (tests/host/nbr_cert_check.cpp runs it under the sanitizers); the
// device side is nbr_cert.hip.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "nngp_math.h"

namespace nngp {

constexpr int kCertInfoLen = 16;                      // NNGP_CERT_INFO_LEN
constexpr int64_t kCertMagic = 0x4e42524345525431ll;  // "NBRCERT1"
// info words
enum {
    kCertIMagic = 0, kCertICoords, kCertINbr, kCertIOrder, kCertINPoints, kCertIDim, kCertINRows, kCertIM, kCertII0,
    kCertITiles, kCertIChecked, kCertISpan  // (the double's bits); 12..15: zero
};
constexpr int kCertMaxM = 24;        // bf_pairb.h kPairbCertMaxM (checked there)
constexpr int kCertTileRows = 128;   // bf_pairb.h kPairbTile
constexpr int kCertSpanBlocks = 256; // blocks of the coordinate pass; 8 doubles each: min[3], max[3], non-finite, 0

// the certificate buffer: a 256-B header (int32 checked-tile count), the checked bits (one per tile, 32 per
// word), the coordinate pass's block records
inline int64_t cert_tiles(int64_t n_rows) { return n_rows > 0 ? (n_rows + kCertTileRows - 1) / kCertTileRows : 0; }
inline size_t cert_align(size_t b) { return (b + 255) & ~(size_t)255; }
constexpr size_t kCertMaskOff = 256;
inline size_t cert_mask_bytes(int64_t tiles) { return cert_align((size_t)((tiles + 31) / 32) * 4); }
inline size_t cert_span_off(int64_t tiles) { return kCertMaskOff + cert_mask_bytes(tiles); }
inline size_t cert_total_bytes(int64_t n_rows) {
    return cert_span_off(cert_tiles(n_rows)) + (size_t)kCertSpanBlocks * 8 * sizeof(double);
}

// a slot that makes its tile checked
NNGP_HD bool cert_slot_checked(int32_t j, int64_t n_points) { return j < 0 || (int64_t)j >= n_points; }

// tile t of (tiles, q, rem) holds q + (t < rem) rows from t q + min(t, rem) (bf_pairb.h pairb_tiling)
inline int64_t cert_tile_row0(int64_t t, int64_t q, int64_t rem) { return t * q + (t < rem ? t : rem); }

// host reference of the device pass (nbr_cert.hip cert_tiles_kernel): the checked bits and their count
inline int64_t cert_mask_host(const int32_t* nbr, int64_t n_rows, int m, int64_t n_points, uint32_t* mask) {
    const int64_t T = cert_tiles(n_rows);
    for (int64_t w = 0; w < (T + 31) / 32; ++w) mask[w] = 0;
    if (T == 0) return 0;
    const int64_t q = n_rows / T, rem = n_rows % T;
    int64_t checked = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t r0 = cert_tile_row0(t, q, rem), rows = q + (t < rem ? 1 : 0);
        bool any = false;
        for (int64_t r = r0; r < r0 + rows && !any; ++r)
            for (int s = 0; s < m && !any; ++s) any = cert_slot_checked(nbr[r * m + s], n_points);
        if (any) {
            mask[t >> 5] |= 1u << (t & 31);
            ++checked;
        }
    }
    return checked;
}

// d2_span from the coordinate pass's block records; false: a coordinate was not finite
inline bool cert_span_fold(const double* rec, int n_blocks, int dim, double* d2_span) {
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool finite = true;
    for (int b = 0; b < n_blocks; ++b) {
        for (int c = 0; c < dim; ++c) {
            mn[c] = fmin(mn[c], rec[8 * b + c]);
            mx[c] = fmax(mx[c], rec[8 * b + 3 + c]);
        }
        finite = finite && rec[8 * b + 6] == 0.0;
    }
    double s = 0.0;
    for (int c = 0; c < dim; ++c) {
        const double e = mx[c] - mn[c];
        s += e * e;
    }
    *d2_span = s;
    return finite && isfinite(s);
}

inline double cert_info_span(const int64_t* info) {
    double s;
    memcpy(&s, &info[kCertISpan], sizeof s);
    return s;
}

// Tiles a sweep of (kind, theta) runs trusted -- the one theta-dependent decision.  The trusted instance drops
// x = fmin(d2, d2max): the identity when every d2 it sees is below d2max.  A computed d2 (D FMAs plus the 2^-1000
// floor) and the computed span each carry a few ulp; the factor 1 + 2^-40 covers both a million times over.  The
// spherical kind's result does not depend on its clamp (past the range u = min(phi d, 1) is 1 either way), so
// it only needs a finite span.
inline int64_t cert_trusted_tiles(const int64_t* info, int kind, double sigma2, double phi, double tau2) {
    if (info == nullptr || info[kCertIMagic] != kCertMagic) return 0;
    if (kind < 0 || kind > 4) return 0;
    if (info[kCertIM] < 1 || info[kCertIM] > kCertMaxM || info[kCertIDim] < 1 || info[kCertIDim] > 3) return 0;
    if (!(sigma2 > 0.0) || !(phi > 0.0) || !(tau2 >= 0.0) || !isfinite(sigma2) || !isfinite(phi) || !isfinite(tau2))
        return 0;
    const double span = cert_info_span(info) * (1.0 + 0x1p-40);
    if (!(span >= 0.0) || !isfinite(span)) return 0;
    if (kind != NNGP_KIND_SPHERICAL) {
        const CovParams P = nngp_cov_params_unit(kind, phi, tau2 / sigma2);
        if (!(span < P.d2max)) return 0;
    }
    const int64_t t = info[kCertITiles] - info[kCertIChecked];
    return t > 0 ? t : 0;
}

}  // namespace nngp
