// Stand-alone driver of csrc/gate_ring.hpp (the dirty-frame rule, the ring slots, the tile plan and the scratch / cache sizes of
// rvcmi_glue_spectral_gate_ring_batch) for tests/test_cpu_gate_ring.py: built with a plain C++ compiler under -fsanitize=address,undefined
// together with csrc/error.cpp, run as a child process.  Prints one "ok <case>" line per case and "gate ring ok" at the end; the first
// failed expectation prints what it saw and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../retrieval-based-voice-conversion-webui_amd/csrc/gate_ring.hpp"

using namespace rvcmi;

namespace {

void expect(const char* what, bool ok) {
    if (!ok) {
        printf("FAILED %s\n", what);
        exit(1);
    }
    printf("ok %s\n", what);
}

}  // namespace

int main() {
    GateRingPlan p;
    // the realtime GUI at 48 kHz: zc = 480, n_fft = 4 zc, hop = zc, the rolling buffer 281 zc, a block 25 zc
    expect("gui plan", gate_ring_plan(281 * 480, 1920, 480, 25 * 480, 25 * 480, &p) && p.Fn == 282 && p.K == 961 && p.head == 2 && p.back == 255 &&
                           p.advance == 25 && p.n_dirty == 29 && p.tiles_dirty == 4 && p.tiles_cold == 36);
    expect("gui plan, input gate on", gate_ring_plan(281 * 480, 1920, 480, 25 * 480, 27 * 480, &p) && p.n_dirty == 31 && p.back == 253);
    expect("a tail shorter than the shift counts as the shift", gate_ring_plan(281 * 480, 1920, 480, 25 * 480, 0, &p) && p.n_dirty == 29);

    // everything dirty: the cold arithmetic, not a refusal
    const int64_t bad[][2] = {{7, 7}, {-16, 0}, {16, 1000}, {2000, 2000}};
    bool all = true;
    for (auto& b : bad) all = all && gate_ring_plan(640, 64, 16, b[0], b[1], &p) && p.head == p.Fn && p.back == p.Fn && p.n_dirty == p.Fn && p.advance == 0;
    expect("off-hop / negative shift, tail > nn, shift > nn: every frame dirty", all);
    expect("a buffer shorter than a frame: every frame dirty", gate_ring_plan(40, 64, 16, 16, 16, &p) && p.n_dirty == p.Fn && p.Fn == 3);
    expect("shift 0, tail 0: nothing dirty", gate_ring_plan(640, 64, 16, 0, 0, &p) && p.n_dirty == 0 && p.tiles_dirty == 0 && p.head == 0 && p.back == p.Fn);
    expect("shift 0, tail 16: the back only", gate_ring_plan(640, 64, 16, 0, 16, &p) && p.head == 0 && p.back == 38 && p.n_dirty == 3);

    // the dirty list is the head, then the back, each frame once and only dirty ones
    gate_ring_plan(640, 64, 16, 48, 48, &p);
    bool list_ok = p.n_dirty == p.head + p.Fn - p.back;
    std::vector<int> seen(p.Fn, 0);
    for (int j = 0; j < p.n_dirty; ++j) {
        const int f = gate_ring_dirty_frame(p, j);
        list_ok = list_ok && f >= 0 && f < p.Fn && gate_ring_is_dirty(p, f) && !seen[f]++;
    }
    for (int f = 0; f < p.Fn; ++f) list_ok = list_ok && (seen[f] == 1) == gate_ring_is_dirty(p, f);
    expect("dirty list", list_ok);

    // ring slots: a clean frame f of this call sits where frame f + advance of the previous call was written; the slots of one call are a
    // permutation; wrap-around and negative bases
    bool slots = true;
    int64_t base = 0;
    for (int step = 0; step < 50; ++step) {
        const int64_t prev = base;
        base += p.advance;
        for (int f = p.head; f < p.back; ++f) slots = slots && gate_ring_slot(base, f, p.Fn) == gate_ring_slot(prev, f + p.advance, p.Fn);
        std::vector<int> used(p.Fn, 0);
        for (int f = 0; f < p.Fn; ++f) {
            const int s = gate_ring_slot(base, f, p.Fn);
            slots = slots && s >= 0 && s < p.Fn && !used[s]++;
        }
    }
    expect("ring slots follow the roll and wrap", slots && base > 3 * p.Fn);
    expect("negative and huge bases", gate_ring_slot(-1, 0, 41) == 40 && gate_ring_slot(-41, 5, 41) == 5 &&
                                          gate_ring_slot(((int64_t)1 << 40) + 3, 40, 41) == (int)((((int64_t)1 << 40) + 43) % 41));

    // sizes
    expect("ring bytes", gate_ring_bytes(64, 281 * 480, 1920, 480) == (size_t)64 * 282 * 961 * 16 && gate_ring_bytes(1, 16, 8, 2) == (size_t)9 * 5 * 16);
    GateRingLayout g;
    bool lay = gate_ring_layout(3, 100, 8, 2, &g) && g.F == 51 && g.K == 5 && g.tiles_x == 7;
    lay = lay && g.x == 0 && g.xmax == align256((size_t)3 * 51 * 5 * 16) && g.thresh == g.xmax + align256(3 * 5 * 8) &&
          g.mask == g.thresh + align256(3 * 5 * 8) && g.frames == g.mask + align256((size_t)3 * 51 * 5 * 4) &&
          g.total == g.frames + align256((size_t)3 * 51 * 8 * 8);
    lay = lay && g.xmax % 256 == 0 && g.thresh % 256 == 0 && g.mask % 256 == 0 && g.frames % 256 == 0 && g.total % 256 == 0;
    expect("scratch layout", lay);

    // refusals
    expect("refused: S = 0 / S too large", !gate_ring_layout(0, 100, 8, 2, &g) && !gate_ring_layout(65536, 100, 8, 2, &g) && gate_ring_bytes(0, 100, 8, 2) == 0 &&
                                               gate_ring_bytes(65536, 100, 8, 2) == 0);
    expect("refused: odd n_fft", !gate_ring_plan(100, 9, 2, 2, 2, &p) && !gate_ring_layout(1, 100, 9, 2, &g) && gate_ring_bytes(1, 100, 9, 2) == 0);
    expect("refused: n_fft > 4096", !gate_ring_plan(100000, 4098, 1024, 0, 0, &p) && gate_ring_bytes(1, 100000, 4098, 1024) == 0);
    expect("refused: hop outside [1, n_fft]", !gate_ring_plan(100, 8, 0, 0, 0, &p) && !gate_ring_plan(100, 8, 9, 0, 0, &p) && !gate_ring_layout(1, 100, 8, 9, &g));
    expect("refused: empty signals", !gate_ring_plan(0, 8, 2, 0, 0, &p) && !gate_ring_layout(1, 0, 8, 2, &g) && gate_ring_bytes(1, 0, 8, 2) == 0);
    expect("refused: too many frames", !gate_ring_layout(1, (int64_t)65535 * 2, 8, 2, &g) && gate_ring_layout(1, (int64_t)65534 * 2, 8, 2, &g));
    printf("gate ring ok\n");
    return 0;
}
