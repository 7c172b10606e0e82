// widgets.cuh — the custom-gate constraint polynomials of the reference
// prover (plonk-core/src/proof_system/widget: GateConstraint::constraints),
// host + device: the quotient evaluates selector(x) * constraints(values at x)
// per coset point (k_widgets_, protocol.hip), the linearisation scales the
// selector polynomial by constraints(evaluations at z) on the host
// (widget/mod.rs:83-104).
#pragma once
#include "field.cuh"

namespace pnp {

struct WidgetVals {
    Fr a, b, c, d;              // wire values
    Fr a_next, b_next, d_next;  // wire values of the next row (w x)
    Fr q_l, q_r, q_c;           // selector values
};

// Jubjub (ark-ed-on-bls12-381): a = -1, d = -10240/10241, Montgomery
PNP_HD Fr jj_coeff_a() {
    Fr r;
    const uint32_t v[8] = {0x3u, 0xfffffffdu, 0xfffb13fcu, 0xfb38ec08u,
                           0x1ce5880fu, 0x99ad8818u, 0x7cd877d8u, 0x5bc8f5f9u};
    for (int i = 0; i < 8; i++) r.v[i] = v[i];
    return r;
}
PNP_HD Fr jj_coeff_d() {
    Fr r;
    const uint32_t v[8] = {0xb974f6b0u, 0x2a522455u, 0x0d9acab3u, 0xfc6cc9efu,
                           0xc27628d1u, 0x7a08fb94u, 0xfe0e262eu, 0x57f8f6a8u};
    for (int i = 0; i < 8; i++) r.v[i] = v[i];
    return r;
}

PNP_HD Fr mul4(const Fr &x) { return dbl(dbl(x)); }

// delta(f) = f (f - 1)(f - 2)(f - 3)  (range.rs:66-74, logic.rs:84-93)
PNP_HD Fr gate_delta(const Fr &f) {
    const Fr one = Fr::one();
    const Fr f1 = f - one, f2 = f1 - one, f3 = f2 - one;
    return f * f1 * f2 * f3;
}

// The constraints of one family, each on its own: c_*(w, emit) hands
// constraint k of the family, without its power of the separation challenge,
// to emit(CIdx<k>{}, value), in the widget's order.  The row-by-row
// satisfiability check (check.hip) tests each value against zero; w_* below,
// what the quotient and the linearisation use, are their kappa-weighted sums,
// taken as the values arrive (no value is kept).
template <int K>
struct CIdx {
    static constexpr int value = K;
};
constexpr int kRangeConstraints = 4, kLogicConstraints = 5, kFbsmConstraints = 4, kCaddConstraints = 3;

// Range (widget/range.rs:44-60)
template <class Emit>
PNP_HD void c_range(const WidgetVals &w, Emit &&emit) {
    emit(CIdx<0>{}, gate_delta(w.c - mul4(w.d)));
    emit(CIdx<1>{}, gate_delta(w.b - mul4(w.c)));
    emit(CIdx<2>{}, gate_delta(w.a - mul4(w.b)));
    emit(CIdx<3>{}, gate_delta(w.d_next - mul4(w.a)));
}

// Range::constraints
PNP_HD Fr w_range(const Fr &sep, const WidgetVals &w) {
    const Fr kappa = sep * sep, kappa2 = kappa * kappa, kappa3 = kappa2 * kappa;
    Fr acc = Fr::zero();
    c_range(w, [&](auto k, const Fr &v) {
        constexpr int K = decltype(k)::value;
        if constexpr (K == 0) acc = v;
        else acc += v * (K == 1 ? kappa : K == 2 ? kappa2 : kappa3);
    });
    return acc * sep;
}

// delta_xor_and (widget/logic.rs:104-133), small constants by additions
PNP_HD Fr delta_xor_and(const Fr &a, const Fr &b, const Fr &w, const Fr &c, const Fr &q_c) {
    const Fr one = Fr::one();
    const Fr two = dbl(one), three = two + one, four = dbl(two), nine = dbl(four) + one;
    const Fr eighteen = dbl(nine), eighty_one = mul4(eighteen) + nine, eighty_three = eighty_one + two;
    const Fr apb = a + b;
    Fr F = w * (w * (four * w - eighteen * apb + eighty_one) + eighteen * (a * a + b * b) -
                eighty_one * apb + eighty_three);
    Fr E = three * (apb + c) - dbl(F);
    Fr B = q_c * (nine * c - three * apb);
    return B + E;
}

// Logic (widget/logic.rs:59-82)
template <class Emit>
PNP_HD void c_logic(const WidgetVals &w, Emit &&emit) {
    const Fr a = w.a_next - mul4(w.a), b = w.b_next - mul4(w.b), d = w.d_next - mul4(w.d);
    emit(CIdx<0>{}, gate_delta(a));
    emit(CIdx<1>{}, gate_delta(b));
    emit(CIdx<2>{}, gate_delta(d));
    emit(CIdx<3>{}, w.c - a * b);
    emit(CIdx<4>{}, delta_xor_and(a, b, w.c, d, w.q_c));
}

// Logic::constraints
PNP_HD Fr w_logic(const Fr &sep, const WidgetVals &w) {
    const Fr kappa = sep * sep, kappa2 = kappa * kappa, kappa3 = kappa2 * kappa, kappa4 = kappa3 * kappa;
    Fr acc = Fr::zero();
    c_logic(w, [&](auto k, const Fr &v) {
        constexpr int K = decltype(k)::value;
        if constexpr (K == 0) acc = v;
        else acc += v * (K == 1 ? kappa : K == 2 ? kappa2 : K == 3 ? kappa3 : kappa4);
    });
    return acc * sep;
}

// FixedBaseScalarMul (widget/ecc/fixed_base_scalar_mul.rs:89-155): bit
// consistency, xy_alpha, the x and the y equation
template <class Emit>
PNP_HD void c_fbsm(const WidgetVals &w, Emit &&emit) {
    const Fr one = Fr::one();
    const Fr bit = w.d_next - dbl(w.d);                   // extract_bit
    emit(CIdx<0>{}, bit * (bit - one) * (bit + one));     // check_bit_consistency
    const Fr y_alpha = bit * bit * (w.q_r - one) + one;   // y_beta = q_r
    const Fr x_alpha = w.q_l * bit;                       // x_beta = q_l
    emit(CIdx<1>{}, bit * w.q_c - w.c);                   // xy_alpha = c
    const Fr m = w.c * w.a * w.b * jj_coeff_d();          // xy_alpha acc_x acc_y D
    emit(CIdx<2>{}, w.a_next + w.a_next * m - (x_alpha * w.b + y_alpha * w.a));
    emit(CIdx<3>{}, w.b_next - w.b_next * m - (y_alpha * w.b - jj_coeff_a() * x_alpha * w.a));
}

// FixedBaseScalarMul::constraints
PNP_HD Fr w_fbsm(const Fr &sep, const WidgetVals &w) {
    const Fr kappa = sep * sep, kappa2 = kappa * kappa, kappa3 = kappa2 * kappa;
    Fr acc = Fr::zero();
    c_fbsm(w, [&](auto k, const Fr &v) {
        constexpr int K = decltype(k)::value;
        if constexpr (K == 0) acc = v;
        else acc += v * (K == 1 ? kappa : K == 2 ? kappa2 : kappa3);
    });
    return acc * sep;
}

// CurveAddition (widget/ecc/curve_addition.rs:61-96): x1 y2, the x3 and the y3 equation
template <class Emit>
PNP_HD void c_cadd(const WidgetVals &w, Emit &&emit) {
    const Fr &x1 = w.a, &y1 = w.b, &x2 = w.c, &y2 = w.d, &x3 = w.a_next, &y3 = w.b_next,
             &x1y2 = w.d_next;
    emit(CIdx<0>{}, x1 * y2 - x1y2);
    const Fr y1x2 = y1 * x2, y1y2 = y1 * y2, x1x2 = x1 * x2;
    const Fr dm = jj_coeff_d() * x1y2 * y1x2;
    emit(CIdx<1>{}, x1y2 + y1x2 - (x3 + x3 * dm));
    emit(CIdx<2>{}, y1y2 - jj_coeff_a() * x1x2 - (y3 - y3 * dm));
}

// CurveAddition::constraints
PNP_HD Fr w_cadd(const Fr &sep, const WidgetVals &w) {
    const Fr kappa = sep * sep;
    Fr acc = Fr::zero();
    c_cadd(w, [&](auto k, const Fr &v) {
        constexpr int K = decltype(k)::value;
        if constexpr (K == 0) acc = v;
        else acc += v * (K == 1 ? kappa : kappa * kappa);
    });
    return acc * sep;
}

}  // namespace pnp
