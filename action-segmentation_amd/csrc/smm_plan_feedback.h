// smm_plan_feedback.h -- the stream split of a decode, planned from MEASURED per-video DP times (smm_api.hip: plan feedback).
// Plain C++: no HIP types, no library state -- a stand-alone program can compile it (tests/plan_feedback_main.cpp).
//
// The replay.  A split decode runs [emission of the first part | DP of the first part] on the caller's stream and
// [emission of the rest | DP of the rest] on a second stream that forks behind the first part's emission.  Emission
// takes em_us for the whole corpus, shared out by frames.  In the model
//   - a video of the first part has a CU to itself (n1 <= n_cu / 2) and runs from em1 = em_us x its part's share of the
//     frames to em1 + its measured time;
//   - the rest starts when all of the emission is through, at em_us, on the n_cu - n1 CUs the first part leaves; the first
//     part's CUs join as they come free; a workgroup goes to the CU that is free first, in launch order (list scheduling);
//   - the step ends with its last video.
// The planner tries, for every size n1 the guards of choose_split admit, the first part made of the n1 videos with the
// LARGEST measured times, both parts launched longest first, and keeps the size whose replay ends first.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <numeric>
#include <queue>
#include <vector>

struct SmmFeedbackPlan {
    int n1 = 0;                      // size of the first part
    std::vector<int32_t> order;      // launch order: [first part | rest], both longest measured time first
    double end_current_us = 0.0;     // replayed end of the plan that was measured
    double end_chosen_us = 0.0;      // replayed end of the plan in `order` (= end_current_us when the plan stays)
    bool changed = false;            // false: `order` / n1 are the current plan's
};

// the guards of choose_split (smm_api.hip) on the size of the first part
inline bool smm_feedback_guards(int b, int n_cu, int n1)
{
    return b >= 24 && n_cu > 0 && n1 >= 1 && n1 <= b / 3 && n1 <= n_cu / 2 && b - n1 >= 16;
}

// replayed end (us) of the plan [order[0 .. n1) | order[n1 .. b)]; 0 when the plan is not a split the model covers
inline double smm_feedback_replay(const double *dur_us, const int32_t *frames, const int32_t *order, int b, int n1, int n_cu,
                                  double em_us)
{
    if (b < 1 || n1 < 1 || n1 >= b || n1 >= n_cu) return 0.0;
    double f1 = 0.0, f_all = 0.0;
    for (int i = 0; i < b; ++i) {
        f_all += (double)frames[order[i]];
        if (i < n1) f1 += (double)frames[order[i]];
    }
    const double em1 = f_all > 0.0 ? em_us * f1 / f_all : 0.0;
    double end = 0.0;
    // when each CU comes free for the rest: the first part's as its videos end, the others at once -- so the rest's first
    // n_cu - n1 videos start at em_us, and only what comes after them has to look for the CU that is free first
    std::vector<double> free_at;
    free_at.reserve(n_cu);
    for (int i = 0; i < n1; ++i) {
        const double e = em1 + dur_us[order[i]];
        end = std::max(end, e);
        free_at.push_back(std::max(e, em_us));
    }
    const int direct = std::min(b, n_cu);
    for (int i = n1; i < direct; ++i) {
        const double e = em_us + dur_us[order[i]];
        end = std::max(end, e);
        free_at.push_back(e);
    }
    if (direct < b) {
        std::priority_queue<double, std::vector<double>, std::greater<double>> cus(std::greater<double>(), std::move(free_at));
        for (int i = direct; i < b; ++i) {
            const double e = cus.top() + dur_us[order[i]];
            cus.pop();
            cus.push(e);
            end = std::max(end, e);
        }
    }
    return end;
}

// dur_us / frames: by video; cur_order / cur_n1: the plan the times were measured under; force: take the best plan of the
// planner's own form even where the current one replays no later (tests)
inline SmmFeedbackPlan smm_feedback_plan(const double *dur_us, const int32_t *frames, const int32_t *cur_order, int b, int cur_n1,
                                         int n_cu, double em_us, bool force = false)
{
    SmmFeedbackPlan out;
    out.n1 = cur_n1;
    out.order.assign(cur_order, cur_order + b);
    out.end_current_us = out.end_chosen_us = smm_feedback_replay(dur_us, frames, cur_order, b, cur_n1, n_cu, em_us);
    if (!smm_feedback_guards(b, n_cu, cur_n1)) return out;          // (not a plan choose_split makes: it stays as it is)
    // longest measured time first; equal times keep the current plan's order, so that equal inputs leave the plan alone
    std::vector<int32_t> by_time(cur_order, cur_order + b);
    std::stable_sort(by_time.begin(), by_time.end(), [&](int32_t x, int32_t y) { return dur_us[x] > dur_us[y]; });
    int best_n1 = 0;
    double best_end = 0.0;
    // (the current size first: among sizes that replay alike the plan keeps its size)
    for (int step = 0; step <= b; ++step) {
        const int n1 = step == 0 ? cur_n1 : step;
        if ((step > 0 && n1 == cur_n1) || !smm_feedback_guards(b, n_cu, n1)) continue;
        const double e = smm_feedback_replay(dur_us, frames, by_time.data(), b, n1, n_cu, em_us);
        if (best_n1 == 0 || e < best_end) { best_n1 = n1; best_end = e; }
    }
    if (best_n1 == 0) return out;
    if (!force && !(best_end < out.end_current_us)) return out;
    out.n1 = best_n1;
    out.end_chosen_us = best_end;
    out.changed = best_n1 != cur_n1 || !std::equal(by_time.begin(), by_time.end(), cur_order);
    out.order = std::move(by_time);
    return out;
}
