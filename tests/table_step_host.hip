// Host-side check of csrc/table_step.h, a stand-alone program (its own main, no device work): the launch order, the grid
// composer and the launch loop (tbl_launches) that K7 / K7d / K7s / K7g / K7r / K7f / K7w and their deferred forms share, against
// the loops those launchers spelled out before the header held them (kept here as the reference), for T = 1, 63, 64, 65 and 130 tensors of 0, 1, 8191, 8192, 8193
// and 10^9 elements.  Meant to be built with the host sanitizers and run on a CPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tests/table_step_host.hip -o table_step_host && ./table_step_host
// (tests/test_optim_capi.py does that).  Exit status 0 and "table_step_host ok" when everything holds.
#include "../xdeepfm-pytorch_amd/csrc/table_step.h"

#include <cstdio>
#include <cstdlib>

struct Tensor { long numel; int id; };
struct Dev { long numel; int id; };
template <int N> struct Batch { Dev t[N]; int first[N + 1]; };

#define CHECK(cond, ...) \
    do { if (!(cond)) { std::fprintf(stderr, "table_step_host: " __VA_ARGS__); std::fprintf(stderr, " [%s:%d]\n", __FILE__, __LINE__); std::exit(1); } } while (0)

static const long SIZES[6] = {0, 1, 8191, 8192, 8193, 1000000000L};
static const long BLOCK = 8192;

// ---- the loops as adam_step_impl / opt_step_impl, xdfm_adam_flush and opt_def_grid had them
static std::vector<int> ref_order(const std::vector<Tensor>& ts) {
    const int T = (int)ts.size();
    std::vector<int> order(T);
    for (int t = 0; t < T; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ts[a].numel > ts[b].numel; });
    return order;
}
template <int N>
static void ref_first(Batch<N>& batch, int cnt, int cap) {
    batch.first[0] = 0;
    for (int k = 0; k < N; ++k) {
        long nb = k < cnt ? ceil_div(batch.t[k].numel, (long)BLOCK) : 0;
        if (k < cnt && nb < 1) nb = 1;
        if (nb > cap) nb = cap;
        batch.first[k + 1] = batch.first[k] + (int)nb;
    }
}

template <int N>
static void same(const Batch<N>& a, const Batch<N>& b, int cnt, int cap, const char* what, int T) {
    for (int k = 0; k < N; ++k)
        CHECK(a.t[k].numel == b.t[k].numel && a.t[k].id == b.t[k].id, "%s T=%d: descriptor %d differs from the reference", what, T, k);
    for (int k = 0; k <= N; ++k) CHECK(a.first[k] == b.first[k], "%s T=%d: first[%d] = %d, reference %d", what, T, k, a.first[k], b.first[k]);
    CHECK(a.first[0] == 0, "%s T=%d: first[0] = %d", what, T, a.first[0]);
    for (int k = 0; k < N; ++k) {
        const int nb = a.first[k + 1] - a.first[k];
        CHECK(nb >= 0, "%s T=%d: first[] falls at %d", what, T, k);
        if (k < cnt) CHECK(nb >= 1 && nb <= cap, "%s T=%d: tensor %d of %ld elements got %d blocks (cap %d)", what, T, k, a.t[k].numel, nb, cap);
        else CHECK(nb == 0 && a.t[k].id == a.t[0].id, "%s T=%d: unused descriptor %d got %d blocks or is not t[0]", what, T, k, nb);
    }
}

// a step: sorted, dealt round-robin to ceil(T / N) launches (adam_step_impl with N = 64, opt_step_impl likewise)
template <int N>
static void check_step(const std::vector<Tensor>& ts, int cap) {
    const int T = (int)ts.size();
    const std::vector<int> order = tbl_launch_order(ts.data(), T), want = ref_order(ts);
    CHECK(order == want, "step T=%d: launch order differs from the reference", T);
    std::vector<char> seen(T, 0);
    for (int k = 0; k < T; ++k) {
        CHECK(order[k] >= 0 && order[k] < T && !seen[order[k]], "step T=%d: order is no permutation", T);
        seen[order[k]] = 1;
        if (k) CHECK(ts[order[k - 1]].numel > ts[order[k]].numel || (ts[order[k - 1]].numel == ts[order[k]].numel && order[k - 1] < order[k]),
                     "step T=%d: order is not by falling size, stable", T);
    }
    // the launches as tbl_step_launches composes them: descriptors, grid, first L2 slot and launch number
    const int nlaunch = ceil_div(T, N);
    int taken = 0, slots = 0, launches = 0;
    const int total = tbl_step_launches<Batch<N>>(
        ts.data(), T, [](const Tensor& x) { return Dev{x.numel, x.id}; }, BLOCK, cap, [&](const Batch<N>& got, int got_cnt, int slot0, int l) {
            CHECK(l == launches && l < nlaunch && slot0 == slots, "step T=%d: launch %d (expected %d) starts at slot %d (expected %d)", T, l,
                  launches, slot0, slots);
            Batch<N> ref;
            int cnt = 0;
            for (int k = l; k < T; k += nlaunch) ref.t[cnt++] = Dev{ts[want[k]].numel, ts[want[k]].id};
            CHECK(cnt >= 1 && cnt <= N && cnt == got_cnt, "step T=%d: launch %d holds %d tensors, reference %d", T, l, got_cnt, cnt);
            for (int k = cnt; k < N; ++k) ref.t[k] = ref.t[0];
            ref_first(ref, cnt, cap);
            same(got, ref, cnt, cap, "step", T);
            taken += cnt;
            slots += got.first[cnt];
            ++launches;
        });
    CHECK(taken == T && launches == nlaunch && total == slots, "step T=%d: %d launches hold %d tensors in %d blocks (returned %d)", T, launches,
          taken, slots, total);
}

// a flush / a deferred step: the tensors in their order, N per launch (xdfm_adam_flush with N = 64, opt_def_grid with N = 48)
template <int N>
static void check_chunks(const std::vector<Tensor>& ts, int cap) {
    const int n = (int)ts.size();
    int launches = 0, slots = 0;
    const int total = tbl_launches<Batch<N>>(
        tbl_in_order(n), false, [&](int t) { return Dev{ts[t].numel, ts[t].id}; }, BLOCK, cap, [&](const Batch<N>& got, int got_cnt, int slot0, int l) {
            const int l0 = l * N;
            CHECK(l == launches && l0 < n && slot0 == slots, "chunks T=%d: launch %d (expected %d) starts at slot %d (expected %d)", n, l, launches,
                  slot0, slots);
            Batch<N> ref;
            const int cnt = n - l0 < N ? n - l0 : N;
            CHECK(cnt == got_cnt, "chunks T=%d: launch %d holds %d tensors, reference %d", n, l, got_cnt, cnt);
            for (int k = 0; k < N; ++k) { const Tensor& x = ts[l0 + (k < cnt ? k : 0)]; ref.t[k] = Dev{x.numel, x.id}; }
            ref_first(ref, cnt, cap);
            same(got, ref, cnt, cap, "chunks", n);
            slots += got.first[cnt];
            ++launches;
        });
    CHECK(launches == ceil_div(n, N) && total == slots, "chunks T=%d: %d launches, %d blocks (returned %d)", n, launches, slots, total);
}

int main() {
    const int counts[5] = {1, 63, 64, 65, 130};
    int cases = 0;
    for (int T : counts)
        for (int shift = 0; shift < 6; ++shift) {
            std::vector<Tensor> ts(T);
            for (int t = 0; t < T; ++t) ts[t] = Tensor{SIZES[(t * 5 + shift + t / 6) % 6], t};      // every size, ties far apart
            for (int cap : {512, 4096, 7}) {
                check_step<64>(ts, cap);
                check_chunks<64>(ts, cap);
                check_chunks<48>(ts, cap);
                cases += 3;
            }
        }
    std::printf("table_step_host ok: %d cases\n", cases);
    return 0;
}
