// Test hook: the P-256 field, scalar and point functions the kernels are built from, one call per item, on
// operands the caller chooses. Whole signatures reach this arithmetic only with pseudo-random operands (after the
// first hash or inversion every limb is random), so all-ones limbs, long carry runs, the ends of the Solinas
// overflow and the r >= p fold practically never occur there; here the tests place them.
//
// Every operation reads its operands from flat arrays of little-endian 32-bit words (an fe is 8 words, a jac
// x | y | z, an aff x | y, an xz x | y | zz | zzz) and writes its result to a flat array. Items share no state and
// there is no barrier. The text is instantiated three times: a host loop (csrc/p256_probe.hip, `host`), a kernel
// in csrc/p256_probe.hip under the ILP-first scheduler the verify TU csrc/p256.hip is built with (`ilp`) and a
// kernel in csrc/p256_batch.hip under the default scheduler (`occ`). Each operation calls the existing function
// unchanged; the lane-group operations and their step policies are csrc/p256_steps.h.
//
// The probe checks what the arithmetic computes under each file's device flags. It cannot show that the copy
// inlined into a production kernel is the same machine code; the whole-signature tests stay for that.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "p256_field.h"
#include "p256_sign.h"
#include "p256_steps.h"
#include "p256_verify.h"

namespace upow {
namespace probe {
using namespace p256;

enum Op : int {
    kFeMul, kFeSqr, kFeAdd, kFeSub, kFeNeg, kFeReduce, kFeInv, kFeSqrt, kMulPair,
    kScMontMul, kScToMont, kScFromMont, kScReduce, kScInvSafegcd, kBoothW5,
    kJacDbl, kJacAdd, kJacMadd, kMaddWindow, kJacToAff, kJacToXz,
    kOneLaneDeviceOps,                                   // the operations above run in every mode
    kScInvBgcd = kOneLaneDeviceOps, kScInvFermat,        // host only: the A/B inverse and the host signer's
    kOneLaneOps,
    kMul4 = kOneLaneOps, kSqr4, kDbl4, kAdd4,            // lane groups: `host` and `ilp`, quad or oct policy
    kOps
};

// per item: words of operand a, words of operand b, bytes of result (per lane for the lane-group operations)
struct Shape { const char* name; int a_words, b_words, out_bytes; };
inline Shape shape(int op) {
    static const Shape s[kOps] = {
        {"fe_mul", 8, 8, 32}, {"fe_sqr", 8, 0, 32}, {"fe_add", 8, 8, 32}, {"fe_sub", 8, 8, 32}, {"fe_neg", 8, 0, 32},
        {"fe_reduce", 16, 0, 32}, {"fe_inv", 8, 0, 32}, {"fe_sqrt_candidate", 8, 0, 32}, {"mul_pair", 8, 8, 32},
        {"sc_mont_mul", 8, 8, 32}, {"sc_to_mont", 8, 0, 32}, {"sc_from_mont", 8, 0, 32}, {"sc_reduce", 8, 0, 32},
        {"sc_inv_safegcd_mont", 8, 0, 32}, {"booth_w5", 8, 0, 52},
        {"jac_dbl", 24, 0, 96}, {"jac_add", 24, 24, 96}, {"jac_madd", 24, 16, 96}, {"madd_window", 24, 16, 100},
        {"jac_to_aff", 24, 0, 68}, {"jac_to_xz", 24, 0, 128},
        {"sc_inv_bgcd_mont", 8, 0, 32}, {"sc_inv_mont", 8, 0, 32},
        {"mul4", 32, 32, 128}, {"sqr4", 32, 0, 128}, {"dbl4", 32, 0, 128}, {"add4", 32, 32, 128}};
    return s[op];
}

UPOW_HD fe load_fe(const uint32_t* w) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = w[i];
    return r;
}
UPOW_HD void store_fe(uint8_t* out, int k, const fe& a) {  // the k-th fe of the item's result
    uint32_t* o = reinterpret_cast<uint32_t*>(out) + 8 * k;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = a.v[i];
}
UPOW_HD void store_word(uint8_t* out, int word, uint32_t v) { reinterpret_cast<uint32_t*>(out)[word] = v; }
UPOW_HD jac load_jac(const uint32_t* w) { return jac{load_fe(w), load_fe(w + 8), load_fe(w + 16)}; }
UPOW_HD aff load_aff(const uint32_t* w) { return aff{load_fe(w), load_fe(w + 8)}; }
UPOW_HD xz load_xz(const uint32_t* w) { return xz{load_fe(w), load_fe(w + 8), load_fe(w + 16), load_fe(w + 24)}; }
UPOW_HD void store_jac(uint8_t* out, const jac& p) {
    store_fe(out, 0, p.x);
    store_fe(out, 1, p.y);
    store_fe(out, 2, p.z);
}
UPOW_HD void store_xz(uint8_t* out, const xz& p) {
    store_fe(out, 0, p.x);
    store_fe(out, 1, p.y);
    store_fe(out, 2, p.zz);
    store_fe(out, 3, p.zzz);
}

// One item of a one-lane operation: a and b point at the item's operands, out at its result.
template <int OP>
UPOW_HD void one(const uint32_t* a, const uint32_t* b, uint8_t* out) {
    if constexpr (OP == kFeMul) store_fe(out, 0, fe_mul(load_fe(a), load_fe(b)));
    else if constexpr (OP == kFeSqr) store_fe(out, 0, fe_sqr(load_fe(a)));
    else if constexpr (OP == kFeAdd) store_fe(out, 0, fe_add(load_fe(a), load_fe(b)));
    else if constexpr (OP == kFeSub) store_fe(out, 0, fe_sub(load_fe(a), load_fe(b)));
    else if constexpr (OP == kFeNeg) store_fe(out, 0, fe_neg(load_fe(a)));
    else if constexpr (OP == kFeReduce) {
        uint32_t c[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) c[i] = a[i];
        store_fe(out, 0, fe_reduce(c));
    }
    else if constexpr (OP == kFeInv) store_fe(out, 0, fe_inv(load_fe(a)));
    else if constexpr (OP == kFeSqrt) store_fe(out, 0, fe_sqrt_candidate(load_fe(a)));
    else if constexpr (OP == kMulPair) store_fe(out, 0, mul_pair_host(load_fe(a), load_fe(b)));
    else if constexpr (OP == kScMontMul) store_fe(out, 0, sc_mont_mul(load_fe(a), load_fe(b)));
    else if constexpr (OP == kScToMont) store_fe(out, 0, sc_to_mont(load_fe(a)));
    else if constexpr (OP == kScFromMont) store_fe(out, 0, sc_from_mont(load_fe(a)));
    else if constexpr (OP == kScReduce) store_fe(out, 0, sc_reduce(load_fe(a)));
    else if constexpr (OP == kScInvSafegcd) store_fe(out, 0, sc_inv_safegcd_mont(load_fe(a)));
    else if constexpr (OP == kScInvBgcd) store_fe(out, 0, sc_inv_bgcd_mont(load_fe(a)));
    else if constexpr (OP == kScInvFermat) store_fe(out, 0, sc_inv_mont(load_fe(a)));
    else if constexpr (OP == kBoothW5) {
        BoothW5 bw(load_fe(a));  // digits come top first: digit w goes to byte w
        for (int w = kBoothWindows - 1; w >= 0; --w) out[w] = uint8_t(int8_t(bw.next()));
    }
    else if constexpr (OP == kJacDbl) store_jac(out, jac_dbl(load_jac(a)));
    else if constexpr (OP == kJacAdd) store_jac(out, jac_add(load_jac(a), load_jac(b)));
    else if constexpr (OP == kJacMadd) store_jac(out, jac_madd(load_jac(a), load_aff(b)));
    else if constexpr (OP == kMaddWindow) {
        bool bad = false;
        store_jac(out, madd_window(load_jac(a), load_aff(b), bad));
        store_word(out, 24, bad ? 1u : 0u);
    }
    else if constexpr (OP == kJacToAff) {
        aff q{fe_zero(), fe_zero()};
        const bool ok = jac_to_aff(load_jac(a), q);
        store_word(out, 0, ok ? 1u : 0u);
        store_fe(reinterpret_cast<uint8_t*>(reinterpret_cast<uint32_t*>(out) + 1), 0, q.x);
        store_fe(reinterpret_cast<uint8_t*>(reinterpret_cast<uint32_t*>(out) + 1), 1, q.y);
    }
    else if constexpr (OP == kJacToXz) store_xz(out, jac_to_xz(load_jac(a)));
}

// f(std::integral_constant<int, OP>) for the one-lane operation `op`; false when `op` is not one
template <class F>
inline bool dispatch_one(int op, F&& f) {
    switch (op) {
#define UPOW_PROBE_CASE(K) case K: f(std::integral_constant<int, K>{}); return true;
        UPOW_PROBE_CASE(kFeMul) UPOW_PROBE_CASE(kFeSqr) UPOW_PROBE_CASE(kFeAdd) UPOW_PROBE_CASE(kFeSub)
        UPOW_PROBE_CASE(kFeNeg) UPOW_PROBE_CASE(kFeReduce) UPOW_PROBE_CASE(kFeInv) UPOW_PROBE_CASE(kFeSqrt)
        UPOW_PROBE_CASE(kMulPair) UPOW_PROBE_CASE(kScMontMul) UPOW_PROBE_CASE(kScToMont) UPOW_PROBE_CASE(kScFromMont)
        UPOW_PROBE_CASE(kScReduce) UPOW_PROBE_CASE(kScInvSafegcd) UPOW_PROBE_CASE(kBoothW5) UPOW_PROBE_CASE(kJacDbl)
        UPOW_PROBE_CASE(kJacAdd) UPOW_PROBE_CASE(kJacMadd) UPOW_PROBE_CASE(kMaddWindow) UPOW_PROBE_CASE(kJacToAff)
        UPOW_PROBE_CASE(kJacToXz) UPOW_PROBE_CASE(kScInvBgcd) UPOW_PROBE_CASE(kScInvFermat)
#undef UPOW_PROBE_CASE
        default: return false;
    }
}
template <class F>
inline bool dispatch_group(int op, F&& f) {
    switch (op) {
        case kMul4: f(std::integral_constant<int, kMul4>{}); return true;
        case kSqr4: f(std::integral_constant<int, kSqr4>{}); return true;
        case kDbl4: f(std::integral_constant<int, kDbl4>{}); return true;
        case kAdd4: f(std::integral_constant<int, kAdd4>{}); return true;
        default: return false;
    }
}

// One group of a lane-group operation through the step policy P (QuadHost / OctHost on a host thread, QuadDev /
// OctDev on the group's lanes): the caller runs this on every lane of the group with that lane's own `out`, so
// the result shows what each lane received. mul4 / sqr4: a (and b) hold the four operands of the step's four
// products, out the four products. dbl4 / add4: a and b are XYZZ points, out the whole resulting point.
template <int OP, class P>
UPOW_HD void group(const P& pp, const uint32_t* a, const uint32_t* b, uint8_t* out) {
    if constexpr (OP == kMul4) {
        fe r0, r1, r2, r3;
        pp.mul4(load_fe(a), load_fe(b), load_fe(a + 8), load_fe(b + 8), load_fe(a + 16), load_fe(b + 16),
                load_fe(a + 24), load_fe(b + 24), r0, r1, r2, r3);
        store_xz(out, xz{r0, r1, r2, r3});
    } else if constexpr (OP == kSqr4) {
        fe r0, r1, r2, r3;
        pp.sqr4(load_fe(a), load_fe(a + 8), load_fe(a + 16), load_fe(a + 24), r0, r1, r2, r3);
        store_xz(out, xz{r0, r1, r2, r3});
    } else if constexpr (OP == kDbl4) {
        xz p = load_xz(a);
        dbl4(pp, p);
        store_xz(out, p);
    } else if constexpr (OP == kAdd4) {
        xz p = load_xz(a);
        add4(pp, p, load_xz(b));
        store_xz(out, p);
    }
}

}  // namespace probe
}  // namespace upow
