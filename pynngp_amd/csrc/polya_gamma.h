// Polya-Gamma draws omega ~ PG(b, c) (Polson, Scott and Windle 2013), the augmentation that makes a
// binomial / logistic NNGP conditionally Gaussian: __host__ __device__, so the kernels (polya_gamma.hip)
// and a CPU check program (tests/host/pg_check.cpp) run the same source.
//
// PG(1, c) = J*(1, z = |c| / 2) / 4 by Devroye's exact method with truncation point t = 0.64 and
// K = pi^2 / 8 + z^2 / 2:
//   proposal  X = t + Exp(1) / K with probability p / (p + q), else the inverse Gaussian IG(1 / z, 1)
//             truncated to (0, t];  p = (pi / 2K) e^{-K t},  q = 2 e^{-z} P(IG(1 / z, 1) <= t).
//             q / p is formed in log space, (4 / pi) (e^{xb} + e^{xa}) with
//             xb = log K + K t - z + log Phi((t z - 1) / sqrt t), xa = log K + K t + z + log Phi(-(t z + 1) / sqrt t):
//             e^{2z} Phi(.) is never formed (log Phi by its asymptotic series below -30), so nothing
//             overflows before the final exp, whose +inf gives the probability 0 it should.
//   truncated IG: z t < 1 (mean above t, c = 0 included -- 1 / z is never formed): an exponential pair
//             (E1, E2) with E1^2 <= 2 E2 / t gives X = t / (1 + t E1)^2, accepted with probability
//             e^{-z^2 X / 2};  otherwise the chi^2 transformation of IG(mu = 1 / z, 1), the root taken in
//             its cancellation-free form mu / (1 + w + sqrt(w (2 + w))), w = mu Y / 2, rejected while X > t.
//   accept    the alternating series S_n = sum (-1)^k a_k(X) against Y = U a_0(X): accept at the first odd n
//             with Y <= S_n, reject at the first even n with Y > S_n; a_n in its left form for X <= t, its
//             right form for X > t.
// PG(b, c), integer 0 <= b <= NNGP_PG_MAX_TRIALS, is the sum of b PG(1, c) draws added in draw order; b = 0
// gives exactly 0.0.  (A saddle-point or normal approximation for large b is out of scope.)
//
// Random numbers: Philox4x32-10 (philox.h), key = seed, counter = (location, sweep'),
//   sweep' = iteration | 1 << 62 | j << 40,   j = 0, 1, 2, ... the location's next 128-bit block:
// bit 63 is clear (update_y_unobserved sets it) and bit 62 set (the w sweep's counters are the bare iteration,
// below 2^40), so no block of the other streams is reused.  A block yields two 53-bit uniforms in (0, 1) made as
// philox_normal makes them; exponentials are -log u, normals Box-Muller.  A draw is a function of
// (seed, iteration, location, b, c) alone -- not of n, the grid or the neighbours in the wave.
//
// Every loop is bounded (kPgCap rounds: the proposal loop -- a proposal is accepted with probability above
// 0.999 --, each truncated-IG loop, the series loop, which decides within a handful of terms): a NaN makes
// every comparison false and would otherwise spin for ever.  A non-finite c or a b outside
// [0, NNGP_PG_MAX_TRIALS] is detected before any loop.  Such a location, or one that hits a cap, gets NaN and
// *bad = true (the kernels report its index through a status word).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/nngp.h"
#include "philox.h"

namespace nngp {

constexpr int kPgCap = 256;
constexpr double kPgT = 0.64;
constexpr double kPgPi = 3.141592653589793;

// NNGP_PG_COUNT (the CPU check program): the stream also records the loop rounds it took
struct PgStream {
    uint64_t seed, loc, iter;
    uint32_t j;
#ifdef NNGP_PG_COUNT
    int max_prop, max_ig, max_series;
    long long blocks;
#endif
};
#ifdef NNGP_PG_COUNT
#define NNGP_PG_NOTE(s, field, v) ((s).field = (v) > (s).field ? (v) : (s).field)
#else
#define NNGP_PG_NOTE(s, field, v) ((void)0)
#endif

NNGP_PHILOX_HD void pg_next2(PgStream& s, double* u1, double* u2) {
    const uint64_t sweep = s.iter | (1ull << 62) | ((uint64_t)(s.j & 0x3FFFFFu) << 40);
    ++s.j;
#ifdef NNGP_PG_COUNT
    ++s.blocks;
#endif
    philox_uniform2(s.seed, s.loc, sweep, u1, u2);
}

// log Phi(x): erfc down to -30 (erfc(21.2) ~ 1e-197, no underflow), below it the asymptotic series
// (next term 945 / x^10 < 2e-12 relative)
NNGP_PHILOX_HD double pg_log_pnorm(double x) {
    if (x > -30.0) return log(0.5 * erfc(-0.7071067811865476 * x));
    const double i2 = 1.0 / (x * x);
    return -0.5 * x * x - log(-x) - 0.9189385332046727 +
           log1p(-i2 * (1.0 - 3.0 * i2 * (1.0 - 5.0 * i2 * (1.0 - 7.0 * i2))));
}

// p / (p + q): the probability of the exponential right tail
NNGP_PHILOX_HD double pg_tail_mass(double z, double K) {
    const double b = 1.25 * (kPgT * z - 1.0), a = -1.25 * (kPgT * z + 1.0);  // 1 / sqrt(0.64) = 1.25
    const double x0 = log(K) + K * kPgT;
    const double xb = x0 - z + pg_log_pnorm(b);
    const double xa = x0 + z + pg_log_pnorm(a);
    return 1.0 / (1.0 + 1.2732395447351628 * (exp(xb) + exp(xa)));
}

// IG(1 / z, 1) truncated to (0, t]
NNGP_PHILOX_HD double pg_rtigauss(double z, PgStream& s, bool* bad) {
    double u1, u2, v, v2;
    if (z * kPgT < 1.0) {
        for (int k = 1; k <= kPgCap; ++k) {
            pg_next2(s, &u1, &u2);
            const double e1 = -log(u1), e2 = -log(u2);
            if (e1 * e1 <= 2.0 * e2 / kPgT) {
                double x = 1.0 + e1 * kPgT;
                x = kPgT / (x * x);
                pg_next2(s, &v, &v2);
                if (v <= exp(-0.5 * z * z * x)) {
                    NNGP_PG_NOTE(s, max_ig, k);
                    return x;
                }
            }
        }
    } else {
        const double mu = 1.0 / z;
        for (int k = 1; k <= kPgCap; ++k) {
            pg_next2(s, &u1, &u2);
            const double y = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
            const double w = 0.5 * mu * y * y;
            double x = mu / (1.0 + w + sqrt(w * (2.0 + w)));
            pg_next2(s, &v, &v2);
            if (v > mu / (mu + x)) x = mu * mu / x;
            if (x <= kPgT) {
                NNGP_PG_NOTE(s, max_ig, k);
                return x;
            }
        }
    }
    NNGP_PG_NOTE(s, max_ig, kPgCap + 1);
    *bad = true;
    return NAN;
}

// one PG(1, 2z) draw; K = pi^2 / 8 + z^2 / 2 and mass = pg_tail_mass(z, K) are the caller's (shared by the b draws)
NNGP_PHILOX_HD double pg_draw1(double z, double K, double mass, PgStream& s, bool* bad) {
    for (int round = 1; round <= kPgCap; ++round) {
        double u0, uy, e, e2;
        pg_next2(s, &u0, &uy);
        double x;
        if (u0 < mass) {
            pg_next2(s, &e, &e2);
            x = kPgT + -log(e) / K;
        } else {
            x = pg_rtigauss(z, s, bad);
            if (*bad) return NAN;
        }
        // a_n(x) = pi (n + 1/2) e^{-(n + 1/2)^2 pi^2 x / 2} for x > t (right),
        //          pi (n + 1/2) (2 / (pi x))^{3/2} e^{-2 (n + 1/2)^2 / x} for x <= t (left)
        const bool right = x > kPgT;
        const double lead = right ? 0.0 : -1.5 * log(0.5 * kPgPi * x);
        const double rate = right ? -0.5 * kPgPi * kPgPi * x : -2.0 / x;
        double S = 0.5 * kPgPi * exp(lead + rate * 0.25);
        const double Y = uy * S;
        int verdict = 0;  // 1 accept, -1 reject, 0 undecided at the cap
        for (int n = 1; n <= kPgCap; ++n) {
            const double h = n + 0.5;
            const double an = h * kPgPi * exp(lead + rate * h * h);
            if (n & 1) {
                S -= an;
                if (Y <= S) verdict = 1;
            } else {
                S += an;
                if (Y > S) verdict = -1;
            }
            if (verdict != 0) {
                NNGP_PG_NOTE(s, max_series, n);
                break;
            }
        }
        if (verdict == 1) {
            NNGP_PG_NOTE(s, max_prop, round);
            return 0.25 * x;
        }
        if (verdict == 0) {
            NNGP_PG_NOTE(s, max_series, kPgCap + 1);
            *bad = true;
            return NAN;
        }
    }
    NNGP_PG_NOTE(s, max_prop, kPgCap + 1);
    *bad = true;
    return NAN;
}

// omega ~ PG(b, c) for (seed, location, iteration).  b outside [0, NNGP_PG_MAX_TRIALS], a non-finite c or a
// loop cap: NaN and *bad = true (b never becomes a trip count unchecked).  b = 0: exactly 0.0, whatever c.
NNGP_PHILOX_HD double pg_draw(int32_t b, double c, PgStream& s, bool* bad) {
    if (b == 0) return 0.0;
    if (b < 0 || b > NNGP_PG_MAX_TRIALS || !(fabs(c) <= 1.7976931348623157e308)) {
        *bad = true;
        return NAN;
    }
    const double z = 0.5 * fabs(c);
    const double K = 0.125 * kPgPi * kPgPi + 0.5 * z * z;
    const double mass = pg_tail_mass(z, K);
    double sum = 0.0;
    for (int32_t k = 0; k < b; ++k) {
        sum += pg_draw1(z, K, mass, s, bad);
        if (*bad) return NAN;
    }
    return sum;
}

NNGP_PHILOX_HD PgStream pg_stream(uint64_t seed, uint64_t loc, uint64_t iteration) {
    PgStream s = {};
    s.seed = seed;
    s.loc = loc;
    s.iter = iteration & ((1ull << 40) - 1);
    return s;
}

}  // namespace nngp
