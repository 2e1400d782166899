// The refusal paths of rrl_se3_adam_step_batch and rrl_register_epoch (include/rrl.h) as a stand-alone host program, for a
// sanitizer build of the library's host side (tools/refusals_sanitize.sh <this file>): the calls of tests/test_register_batch_host.py's
// tables with fake pointers -- every one is refused on the host before a launch, so no pointer is dereferenced and no GPU
// is needed.  Exit status 0: every call returned its documented code.
#include <cstdio>
#include <cstring>
#include <functional>

#include "rrl.h"

static int failures = 0;
static void expect(const char *what, int got, int want) {
    if (got != want) { std::printf("FAIL %s: got %d, want %d\n", what, got, want); ++failures; }
    else std::printf("ok   %s: %d\n", what, got);
}

template <class T> static T *fake(size_t at = 256) { return reinterpret_cast<T *>(at); }

struct StepCall {
    float *xi = fake<float>(), *gR = fake<float>(), *gT = fake<float>(), *m = fake<float>(), *v = fake<float>(), *state = fake<float>(),
          *lr = fake<float>();
    int32_t *gate = fake<int32_t>();
    long long gate_stride = 4;
    float *R = fake<float>(), *T = fake<float>(), *gxi = fake<float>(), *loss = fake<float>(), *value = fake<float>(), *table = fake<float>();
    long long *cursor = fake<long long>();
    long long nrows = 16;
    float *row = fake<float>(), *aabb_rows = fake<float>();
    long long row_stride = 16;
    int32_t *count1 = fake<int32_t>();
    int N = 300;
    float *box = fake<float>();
    int B = 3;
    int run() const {
        return rrl_se3_adam_step_batch(xi, gR, gT, m, v, state, lr, gate, gate_stride, 0.9, 0.999, 1e-8, R, T, gxi, loss, value, table,
                                       cursor, nrows, row, aabb_rows, row_stride, count1, N, box, B, nullptr);
    }
};

static rrl_register_epoch_args epoch_base() {
    rrl_register_epoch_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_bytes = (int32_t)sizeof a;
    a.B = 3; a.N = 300; a.M = 300; a.L = 2048; a.rounds = 10;
    a.rng_state = fake<uint64_t>(); a.radius = fake<float>(); a.centers = fake<float>(); a.box1 = fake<float>(); a.box2 = fake<float>();
    a.lines = fake<float>(); a.filled = fake<int32_t>(); a.tile_counts = fake<int32_t>();
    a.src_tri = fake<float>(); a.tar_tri = fake<float>(); a.R = fake<float>(); a.T = fake<float>(); a.ws = fake<void>();
    a.ws_bytes = (size_t)1 << 50; a.loss = fake<float>(); a.grad_loss = fake<float>(); a.gR = fake<float>(); a.gt = fake<float>();
    a.cham_ws = fake<void>(); a.cham_ws_bytes = (size_t)1 << 50; a.best_x = fake<uint64_t>(); a.best_y = fake<uint64_t>();
    a.cham_mean = fake<float>(); a.value = fake<float>();
    a.xi = fake<float>(); a.m = fake<float>(); a.v = fake<float>(); a.adam_state = fake<float>(); a.lr = fake<float>();
    a.b1 = 0.9; a.b2 = 0.999; a.eps = 1e-8; a.gxi = fake<float>(); a.table = fake<float>(); a.cursor = fake<long long>();
    a.table_rows = 16; a.row = fake<float>();
    return a;
}
static rrl_opts opts_base() {
    rrl_opts o;
    std::memset(&o, 0, sizeof o);
    o.struct_bytes = (int32_t)sizeof o;
    o.reduce_mode = o.deterministic = o.sort_parts = o.scan_variant = -1;
    return o;
}
static void epoch(const char *what, int want, const std::function<void(rrl_register_epoch_args &, rrl_opts &)> &edit) {
    rrl_register_epoch_args a = epoch_base();
    rrl_opts o = opts_base();
    edit(a, o);
    expect(what, rrl_register_epoch(&a, nullptr), want);
}

int main() {
    const int cap1 = rrl_sort_capacity() + 1;
    int32_t *const counts = fake<int32_t>(512);
    { StepCall c; c.xi = nullptr; expect("step: null xi", c.run(), RRL_E_ARG); }
    { StepCall c; c.T = nullptr; expect("step: null T", c.run(), RRL_E_ARG); }
    { StepCall c; c.B = -1; expect("step: negative batch", c.run(), RRL_E_ARG); }
    { StepCall c; c.aabb_rows = nullptr; expect("step: a box without rows", c.run(), RRL_E_ARG); }
    { StepCall c; c.N = 0; expect("step: a box over no capacity", c.run(), RRL_E_ARG); }
    { StepCall c; c.row_stride = 8; expect("step: overlapping rows", c.run(), RRL_E_ARG); }
    { StepCall c; c.gate_stride = -4; expect("step: negative gate stride", c.run(), RRL_E_ARG); }
    { StepCall c; c.B = -1; c.T = nullptr; expect("step: negative batch + null pointer", c.run(), RRL_E_ARG); }
    { StepCall c; c.B = 0; expect("step: an empty batch launches nothing", c.run(), 0); }
    expect("epoch: null struct", rrl_register_epoch(nullptr, nullptr), RRL_E_ARG);
    epoch("epoch: a struct too short", RRL_E_ARG, [](auto &a, auto &) { a.struct_bytes = 64; });
    epoch("epoch: empty batch", RRL_E_ARG, [](auto &a, auto &) { a.B = 0; });
    epoch("epoch: negative size", RRL_E_ARG, [](auto &a, auto &) { a.N = -1; });
    epoch("epoch: no lines", RRL_E_ARG, [](auto &a, auto &) { a.L = 0; });
    epoch("epoch: no sampler rounds", RRL_E_ARG, [](auto &a, auto &) { a.rounds = 0; });
    epoch("epoch: misaligned ballots", RRL_E_ARG, [](auto &a, auto &) { a.tile_counts = fake<int32_t>(260); });
    epoch("epoch: multi-pose", RRL_E_ARG, [](auto &a, auto &o) { a.B = 4; o.problems = 2; a.opts = &o; });
    epoch("epoch: line counts", RRL_E_ARG, [&](auto &a, auto &o) { o.nlines = counts; a.opts = &o; });
    epoch("epoch: the monitor on a ragged batch", RRL_E_ARG, [&](auto &a, auto &o) { o.count1 = o.count2 = counts; a.opts = &o; });
    epoch("epoch: the monitor without its scratch", RRL_E_ARG, [](auto &a, auto &) { a.cham_ws = nullptr; });
    epoch("epoch: the monitor beyond the sort capacity", RRL_E_ARG, [&](auto &a, auto &) { a.N = cap1; });
    epoch("epoch: null xi", RRL_E_ARG, [](auto &a, auto &) { a.xi = nullptr; });
    epoch("epoch: null src_tri", RRL_E_ARG, [](auto &a, auto &) { a.src_tri = nullptr; });
    epoch("epoch: ragged beyond the sort capacity", RRL_E_ARG,
          [&](auto &a, auto &o) { a.N = cap1; a.value = nullptr; o.count1 = o.count2 = counts; a.opts = &o; });
    epoch("epoch: L = 2^24", RRL_E_ARG, [](auto &a, auto &) { a.L = 1 << 24; a.value = nullptr; });
    epoch("epoch: short workspace", RRL_E_WS, [](auto &a, auto &) { a.ws_bytes = 4096; });
    epoch("epoch: short workspace, ragged", RRL_E_WS,
          [&](auto &a, auto &o) { a.ws_bytes = 0; a.value = nullptr; o.count1 = o.count2 = counts; a.opts = &o; });
    epoch("epoch: short Chamfer workspace", RRL_E_WS, [](auto &a, auto &) { a.cham_ws_bytes = 64; });
    epoch("epoch: given lines need no rounds", RRL_E_WS,
          [](auto &a, auto &) { a.rng_state = nullptr; a.rounds = 0; a.radius = nullptr; a.ws_bytes = 0; });
    epoch("epoch: multi-pose + short workspace", RRL_E_ARG, [](auto &a, auto &o) { a.B = 4; o.problems = 2; a.opts = &o; a.ws_bytes = 0; });
    epoch("epoch: null pointer + short workspace", RRL_E_ARG, [](auto &a, auto &) { a.m = nullptr; a.ws_bytes = 0; });
    epoch("epoch: the monitor on a ragged batch + short workspace", RRL_E_ARG,
          [&](auto &a, auto &o) { o.count1 = o.count2 = counts; a.opts = &o; a.ws_bytes = 0; });
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
