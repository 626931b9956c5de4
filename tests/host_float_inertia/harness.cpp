// Host build of the inertia randomisation's arithmetic (csrc/float_task.hpp:
// ft_inertia_scale, ft_inertia_payload), test only: the float32 code the post
// kernel runs per link, with g++ (-DMW_HOST_TEST -ffp-contract=off), and the
// bound on its distance from exact arithmetic on the same float32 inputs.
//
// The bound is derived here from the roundings of the stated operation
// sequence, never from a measured error.  u = 2^-24 is the unit roundoff: a
// rounded operation returns x (1 + d), |d| <= u.  Every quantity in a bound is
// evaluated in double from the float32 inputs; the factor (1 + 16 u) covers
// the second-order terms (at most eight roundings chain up in any word).
//
//   scale, per word               w = fl(s x)                 1 rounding
//       |err| <= u |s x|
//   mass after the payload        m_s = fl(s m0), m1 = fl(m_s + mp)
//       e_m  = u |s m0|           (0 without the scale)
//       |err| <= e_m + u |M|,     M = s m0 + mp
//   centre of mass, per axis      mc = fl(m_s c), num = fmaf(mp, p, mc),
//                                 c' = fl(num / m1)
//       mc:  |c| e_m + u |s m0 c|
//       num: err(mc) + u |N|,     N = s m0 c + mp p
//       c':  (err(num) + |N / M| err(m1)) / M + u |N / M|
//   inertia, diagonal (xx)        I_s = fl(s I0), yy = fl(py py), zz = fl(pz pz),
//                                 S = fl(yy + zz), I' = fmaf(mp, S, I_s)
//       S:   u py^2 + u pz^2 + u (py^2 + pz^2) = 2 u (py^2 + pz^2)
//       I':  mp err(S) + e_I + u |I'|,   e_I = u |s I0| (0 without the scale)
//   inertia, off-diagonal (xy)    xy = fl(px py), I' = fmaf(-mp, xy, I_s)
//       I':  mp u |px py| + e_I + u |I'|
#include "float_task.hpp"

#include <cmath>

namespace {
constexpr double kU = 1.0 / 16777216.0;  // 2^-24
constexpr double kSecond = 1.0 + 16.0 * kU;
}  // namespace

// w0 [count][10], s [count], mp [count], p [count][3]: float32 inputs; flags bit
// 0: scale, bit 1: payload (a feature that is off is skipped, as in the
// kernel).  out [count][10]: the float32 words; bound [count][10]: the derived
// bound on |out - exact|.
extern "C" void fi_apply(int count, int flags, const float* w0, const float* s, const float* mp, const float* p,
                         float* out, double* bound) {
    const bool scale = flags & 1, payload = flags & 2;
    for (int i = 0; i < count; ++i) {
        float a[10], w[10];
        for (int e = 0; e < 10; ++e) w[e] = a[e] = w0[10 * i + e];
        if (scale) mw::dev::ft_inertia_scale(a, s[i], w);
        const float pp[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
        if (payload) mw::dev::ft_inertia_payload(w, mp[i], pp);
        for (int e = 0; e < 10; ++e) out[10 * i + e] = w[e];

        double* b = bound + 10 * i;
        const double sc = scale ? static_cast<double>(s[i]) : 1.0;
        const double m0 = sc * a[0], e_m = scale ? kU * std::fabs(m0) : 0.0;
        if (!payload) {
            b[0] = e_m;
            for (int k = 1; k < 4; ++k) b[k] = 0.0;  // the centre of mass is copied
            for (int k = 4; k < 10; ++k) b[k] = scale ? kU * std::fabs(sc * a[k]) : 0.0;
        } else {
            const double q = mp[i], M = m0 + q;
            const double e_m1 = e_m + kU * std::fabs(M);
            b[0] = e_m1;
            for (int k = 0; k < 3; ++k) {
                const double c = a[1 + k], N = m0 * c + q * pp[k];
                const double e_mc = std::fabs(c) * e_m + kU * std::fabs(m0 * c);
                const double e_num = e_mc + kU * std::fabs(N);
                b[1 + k] = (e_num + std::fabs(N / M) * e_m1) / M + kU * std::fabs(N / M);
            }
            const double x2 = static_cast<double>(pp[0]) * pp[0], y2 = static_cast<double>(pp[1]) * pp[1],
                         z2 = static_cast<double>(pp[2]) * pp[2];
            const double S[3] = {y2 + z2, x2 + z2, x2 + y2};
            const double X[3] = {static_cast<double>(pp[0]) * pp[1], static_cast<double>(pp[0]) * pp[2],
                                 static_cast<double>(pp[1]) * pp[2]};
            for (int k = 0; k < 3; ++k) {
                const double Is = sc * a[4 + k], e_I = scale ? kU * std::fabs(Is) : 0.0;
                b[4 + k] = q * 2.0 * kU * S[k] + e_I + kU * std::fabs(Is + q * S[k]);
                const double Os = sc * a[7 + k], e_O = scale ? kU * std::fabs(Os) : 0.0;
                b[7 + k] = q * kU * std::fabs(X[k]) + e_O + kU * std::fabs(Os - q * X[k]);
            }
        }
        for (int e = 0; e < 10; ++e) b[e] *= kSecond;
    }
}

extern "C" unsigned fi_scale_block(int k) { return mw::dev::ft_scale_block(k); }
extern "C" unsigned fi_payload_block() { return mw::kFtPayloadBlock; }
