// Stand-alone host program for a sanitizer run of the argument checks of combat_cond_fwd / combat_cond_wgrad and
// combat_trigger_groups_fwd / combat_trigger_groups_bwd (include/combat_hip.h): every refused call and the n == 0 no-op
// return before anything is launched, so it needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Icombat_amd/csrc \
//       tools/cond_refusals.cpp combat_amd/csrc/cond.hip combat_amd/csrc/trigger.hip combat_amd/csrc/plan.cpp \
//       combat_amd/csrc/capi.cpp -o cond_refusals
//   ASAN_OPTIONS=detect_leaks=0 ./cond_refusals        (the HIP runtime's own start-up allocations are not the subject)
//
// The buffers are host arrays with the alignment a device buffer would have: the checks look at the pointers' values only.
#include <cstdint>
#include <cstdio>

#include "combat_hip.h"

static int failures = 0;

static void expect(int got, int want, const char *what) {
    if (got != want) {
        std::printf("FAIL %s: returned %d, expected %d\n", what, got, want);
        ++failures;
    }
}

template <typename T>
static T *off(T *p, int bytes) {
    return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + bytes);
}

int main() {
    alignas(16) static float W[64 * 9 * 74], dw[64 * 9 * 74], dwf[64 * 9 * 64], scratch[4 * 9 * 64];
    alignas(16) static int32_t labels[16];
    alignas(16) static uint16_t cond[4 * 16 * 16 * 64], d[4 * 16 * 16 * 64];
    const float *Wy = W + 64;
    const int E = COMBAT_EINVAL;

    auto fwd = [&](const float *w, const int32_t *y, int n, int hw, int nf, int classes, void *out) {
        return combat_cond_fwd(w, y, n, hw, nf, classes, out, nullptr);
    };
    expect(fwd(Wy, labels, 0, 16, 64, 10, cond), COMBAT_OK, "fwd n == 0");
    expect(fwd(Wy, labels, 4, 1, 64, 10, cond), E, "fwd hw_map 1");
    expect(fwd(Wy, labels, 4, 0, 64, 10, cond), E, "fwd hw_map 0");
    expect(fwd(Wy, labels, 4, 1025, 64, 10, cond), E, "fwd hw_map 1025");
    const int bad_nf[] = {0, 4, 24, 48, 72, 512};
    for (int nf : bad_nf) expect(fwd(Wy, labels, 4, 16, nf, 10, cond), E, "fwd nf outside the set");
    expect(fwd(Wy, labels, 4, 16, 64, 0, cond), E, "fwd classes 0");
    expect(fwd(Wy, labels, 4, 16, 64, 1025, cond), E, "fwd classes 1025");
    expect(fwd(Wy, labels, -1, 16, 64, 10, cond), E, "fwd n < 0");
    expect(fwd(nullptr, labels, 4, 16, 64, 10, cond), E, "fwd NULL W_y");
    expect(fwd(Wy, nullptr, 4, 16, 64, 10, cond), E, "fwd NULL labels");
    expect(fwd(Wy, labels, 4, 16, 64, 10, nullptr), E, "fwd NULL cond");
    expect(fwd(off(Wy, 2), labels, 4, 16, 64, 10, cond), E, "fwd W_y + 2");
    expect(fwd(Wy, off(labels, 1), 4, 16, 64, 10, cond), E, "fwd labels + 1");
    expect(fwd(Wy, labels, 4, 16, 64, 10, off(cond, 8)), E, "fwd cond + 8");

    auto wg = [&](const void *g, const int32_t *y, int n, int hw, int nf, int classes, const float *f, float *o, float *s) {
        return combat_cond_wgrad(g, y, n, hw, nf, classes, f, o, s, nullptr);
    };
    expect(wg(d, labels, 0, 16, 64, 10, dwf, dw, scratch), COMBAT_OK, "wgrad n == 0");
    expect(wg(d, labels, 0, 16, 64, 10, nullptr, dw, scratch), COMBAT_OK, "wgrad n == 0, no dwf");
    expect(wg(d, labels, 4, 1, 64, 10, dwf, dw, scratch), E, "wgrad hw_map 1");
    for (int nf : bad_nf) expect(wg(d, labels, 4, 16, nf, 10, dwf, dw, scratch), E, "wgrad nf outside the set");
    expect(wg(d, labels, 4, 16, 64, 0, dwf, dw, scratch), E, "wgrad classes 0");
    expect(wg(d, labels, -1, 16, 64, 10, dwf, dw, scratch), E, "wgrad n < 0");
    expect(wg(nullptr, labels, 4, 16, 64, 10, dwf, dw, scratch), E, "wgrad NULL d");
    expect(wg(d, nullptr, 4, 16, 64, 10, dwf, dw, scratch), E, "wgrad NULL labels");
    expect(wg(d, labels, 4, 16, 64, 10, dwf, nullptr, scratch), E, "wgrad NULL dw");
    expect(wg(d, labels, 4, 16, 64, 10, dwf, dw, nullptr), E, "wgrad NULL scratch");
    expect(wg(off(d, 8), labels, 4, 16, 64, 10, dwf, dw, scratch), E, "wgrad d + 8");
    expect(wg(d, off(labels, 2), 4, 16, 64, 10, dwf, dw, scratch), E, "wgrad labels + 2");
    expect(wg(d, labels, 4, 16, 64, 10, off(dwf, 2), dw, scratch), E, "wgrad dwf + 2");
    expect(wg(d, labels, 4, 16, 64, 10, dwf, off(dw, 1), scratch), E, "wgrad dw + 1");
    expect(wg(d, labels, 4, 16, 64, 10, dwf, dw, off(scratch, 2)), E, "wgrad scratch + 2");

    alignas(16) static float x[3 * 32 * 32], P[32 * 32], k1[6], out[3 * 32 * 32], mse[3];
    alignas(16) static uint16_t noise[32 * 32 * 8], dn[32 * 32 * 8];
    auto tf = [&](const float *xx, const void *nz, const float *pm, const float *k, int n, int hw, int ps, float *o) {
        return combat_trigger_groups_fwd(xx, nz, pm, k, 0.08f, n, hw, ps, o, mse, nullptr);
    };
    expect(tf(x, noise, P, k1, 0, 32, 2, out), COMBAT_OK, "groups fwd n == 0");
    expect(tf(x, noise, P, k1, 1, 32, 0, out), E, "groups fwd ps 0");
    expect(tf(x, noise, P, k1, 1, 32, -3, out), E, "groups fwd ps < 0");
    expect(tf(x, noise, P, k1, 1, 12, 2, out), E, "groups fwd hw 12");
    expect(tf(x, noise, P, k1, 1, 34, 2, out), E, "groups fwd hw 34");
    expect(tf(x, noise, P, k1, 1, 72, 2, out), E, "groups fwd hw 72 (strip route, not a multiple of 16)");
    expect(tf(x, noise, P, k1, 1, 272, 2, out), E, "groups fwd hw 272");
    expect(tf(x, noise, P, k1, 0, 224, 2, out), COMBAT_OK, "groups fwd n == 0 at 224");
    expect(tf(x, noise, P, k1, 1, 224, 0, out), E, "groups fwd ps 0 at 224");
    expect(tf(x, noise, P, k1, -1, 32, 2, out), E, "groups fwd n < 0");
    expect(tf(nullptr, noise, P, k1, 1, 32, 2, out), E, "groups fwd NULL x");
    expect(tf(x, nullptr, P, k1, 1, 32, 2, out), E, "groups fwd NULL noise");
    expect(tf(x, noise, nullptr, k1, 1, 32, 2, out), E, "groups fwd NULL P");
    expect(tf(x, noise, P, nullptr, 1, 32, 2, out), E, "groups fwd NULL k1");
    expect(tf(x, noise, P, k1, 1, 32, 2, nullptr), E, "groups fwd NULL out");

    auto tb = [&](const float *xx, const float *k, int n, int hw, int ps, const float *o, float l2, void *g) {
        return combat_trigger_groups_bwd(xx, noise, P, k, 0.08f, n, hw, ps, out, nullptr, o, l2, 1, g, nullptr);
    };
    expect(tb(x, k1, 0, 32, 2, out, 0.5f, dn), COMBAT_OK, "groups bwd n == 0");
    expect(tb(x, k1, 1, 32, 0, out, 0.5f, dn), E, "groups bwd ps 0");
    expect(tb(x, k1, 1, 8, 2, out, 0.5f, dn), E, "groups bwd hw 8");
    expect(tb(x, k1, 1, 72, 2, out, 0.5f, dn), E, "groups bwd hw 72");
    expect(tb(x, k1, 1, 272, 2, out, 0.5f, dn), E, "groups bwd hw 272");
    expect(tb(x, k1, 0, 224, 2, out, 0.5f, dn), COMBAT_OK, "groups bwd n == 0 at 224");
    expect(tb(x, k1, 1, 224, 2, nullptr, 0.5f, dn), E, "groups bwd L2 term without out at 224");
    expect(tb(x, k1, 1, 32, 2, nullptr, 0.5f, dn), E, "groups bwd L2 term without out");
    expect(tb(nullptr, k1, 1, 32, 2, out, 0.5f, dn), E, "groups bwd NULL x");
    expect(tb(x, nullptr, 1, 32, 2, out, 0.5f, dn), E, "groups bwd NULL k1");
    expect(tb(x, k1, 1, 32, 2, out, 0.5f, nullptr), E, "groups bwd NULL d_noise");

    std::printf(failures ? "%d check(s) failed\n" : "all refusals as declared (%d failures)\n", failures);
    return failures != 0;
}
