// Stand-alone host program for a sanitizer run of the argument checks of combat_gradcam_seed / combat_gradcam_map
// (include/combat_hip.h): every refused call and the n == 0 no-op return before anything is launched, so it needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Icombat_amd/csrc \
//       tools/gradcam_refusals.cpp combat_amd/csrc/gradcam.hip combat_amd/csrc/plan.cpp combat_amd/csrc/capi.cpp -o gradcam_refusals
//   ASAN_OPTIONS=detect_leaks=0 ./gradcam_refusals        (the HIP runtime's own start-up allocations are not the subject)
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

int main() {
    alignas(16) static float logits[16 * 10], W[10 * 512], cam[2 * 32 * 32], raw[2 * 64], weights[2 * 256];
    alignas(16) static int32_t index[16], chosen[16];
    alignas(16) static uint16_t d_feat[16 * 16 * 512], act[2 * 64 * 256], grad[2 * 64 * 256];
    char *fb = reinterpret_cast<char *>(d_feat), *ab = reinterpret_cast<char *>(act), *gb = reinterpret_cast<char *>(grad);
    const int E = COMBAT_EINVAL;

    auto seed = [&](const float *lg, const int32_t *ix, int n, int N, int classes, int C, const float *w, int32_t *ch, void *df) {
        return combat_gradcam_seed(lg, ix, n, N, classes, C, w, ch, df, nullptr);
    };
    expect(seed(logits, index, 0, 16, 10, 512, W, chosen, d_feat), COMBAT_OK, "seed n == 0");
    expect(seed(logits, nullptr, 0, 16, 10, 512, W, chosen, d_feat), COMBAT_OK, "seed n == 0, no index");
    expect(seed(logits, index, 4, 16, 0, 512, W, chosen, d_feat), E, "seed classes 0");
    expect(seed(logits, index, 4, 16, 17, 512, W, chosen, d_feat), E, "seed classes 17");
    expect(seed(logits, index, 4, 16, 10, 12, W, chosen, d_feat), E, "seed C 12");
    expect(seed(logits, index, 4, 16, 10, 0, W, chosen, d_feat), E, "seed C 0");
    expect(seed(logits, index, -1, 16, 10, 512, W, chosen, d_feat), E, "seed n < 0");
    expect(seed(logits, index, 17, 16, 10, 512, W, chosen, d_feat), E, "seed n > N");
    expect(seed(logits, index, 0, 0, 10, 512, W, chosen, d_feat), E, "seed N 0");
    expect(seed(nullptr, index, 4, 16, 10, 512, W, chosen, d_feat), E, "seed NULL logits");
    expect(seed(logits, index, 4, 16, 10, 512, nullptr, chosen, d_feat), E, "seed NULL W");
    expect(seed(logits, index, 4, 16, 10, 512, W, nullptr, d_feat), E, "seed NULL chosen");
    expect(seed(logits, index, 4, 16, 10, 512, W, chosen, nullptr), E, "seed NULL d_feat");
    expect(seed(logits, index, 4, 16, 10, 512, W, chosen, fb + 8), E, "seed d_feat + 8");
    expect(seed(reinterpret_cast<const float *>(reinterpret_cast<const char *>(logits) + 2), index, 4, 16, 10, 512, W, chosen, d_feat),
           E, "seed logits + 2");
    expect(seed(logits, reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(index) + 2), 4, 16, 10, 512, W, chosen, d_feat),
           E, "seed index + 2");

    auto map = [&](const void *a, const void *g, int n, int f, int C, int out_hw, float *c, float *r, float *w) {
        return combat_gradcam_map(a, g, n, f, C, out_hw, c, r, w, nullptr);
    };
    expect(map(act, grad, 0, 8, 256, 32, cam, raw, weights), COMBAT_OK, "map n == 0");
    expect(map(act, grad, 0, 8, 256, 32, cam, nullptr, nullptr), COMBAT_OK, "map n == 0, no optional outputs");
    const int bad_f[] = {0, 2, 3, 12, 64}, bad_c[] = {0, 8, 32, 96, 1024};
    for (int f : bad_f) expect(map(act, grad, 2, f, 256, 32, cam, raw, weights), E, "map f outside the set");
    for (int c : bad_c) expect(map(act, grad, 2, 8, c, 32, cam, raw, weights), E, "map C outside the set");
    expect(map(act, grad, 2, 8, 256, 16, cam, raw, weights), E, "map out_hw 16");
    expect(map(act, grad, -1, 8, 256, 32, cam, raw, weights), E, "map n < 0");
    expect(map(nullptr, grad, 2, 8, 256, 32, cam, raw, weights), E, "map NULL act");
    expect(map(act, nullptr, 2, 8, 256, 32, cam, raw, weights), E, "map NULL grad");
    expect(map(act, grad, 2, 8, 256, 32, nullptr, raw, weights), E, "map NULL cam");
    expect(map(ab + 8, grad, 2, 8, 256, 32, cam, raw, weights), E, "map act + 8");
    expect(map(act, gb + 4, 2, 8, 256, 32, cam, raw, weights), E, "map grad + 4");
    expect(map(act, grad, 2, 8, 256, 32, reinterpret_cast<float *>(reinterpret_cast<char *>(cam) + 2), raw, weights), E, "map cam + 2");
    expect(map(act, grad, 2, 8, 256, 32, cam, reinterpret_cast<float *>(reinterpret_cast<char *>(raw) + 1), weights), E, "map raw + 1");

    std::printf(failures ? "%d check(s) failed\n" : "all refusals as declared (%d failures)\n", failures);
    return failures != 0;
}
