/*
 * stc007_plan_check.cpp - TEST ONLY: the scheduler's decisions for STC-007 tapes (sdvpcmdecoder_amd/csrc/stc007_chain_plan.h) fed by hand, without a tape
 * and without a device.  A stand-alone program (tests/test_stc007_plan.py builds it with -fsanitize=address,undefined and runs it); it prints what it
 * found wrong and returns the number of failed expectations.
 *
 * The expectations are the rules as the plan's comments state them, worked out here by hand - none of them is an output of the code under test.
 */
#define SDV_EMU 1
#include "hip_emu.h"
struct uint4 { uint32_t x, y, z, w; };
struct uint2 { uint32_t x, y; };
#include "../../sdvpcmdecoder_amd/csrc/stc007_device.h"          /* the flag byte a frame leaves: sdv::VF_* */
#include "../../sdvpcmdecoder_amd/csrc/stc007_chain_plan.h"

#include <cstdio>
#include <string>

static int failures = 0;
static const char *current = "";
static std::string show(const std::vector<int> &v) { std::string s = "["; for (size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + std::to_string(v[i]); return s + "]"; }
static void expect(bool ok, const char *what) { if (!ok) { failures++; printf("FAILED %s: %s\n", current, what); } }
static void expect_list(const std::vector<int> &got, const std::vector<int> &want, const char *what)
{
    if (got != want) { failures++; printf("FAILED %s: %s is %s, expected %s\n", current, what, show(got).c_str(), show(want).c_str()); }
}
static std::vector<int> range(int lo, int hi) { std::vector<int> v; for (int k = lo; k < hi; k++) v.push_back(k); return v; }

/* One turn of the driver's loop without its device: the steps in the driver's order.  Returns whether a round is to be run; asked_sig / asked_refs: the
 * plan wanted the give-up signatures / the reference levels read back. */
struct Turn { bool round, asked_sig, asked_refs; };
static Turn turn(ChainPlan &p, const std::vector<uint8_t> &flag, const uint8_t *sig, const uint8_t *refs)
{
    Turn t = { false, false, false };
    if (ChainPlan::all_links_hold(flag.data(), p.first, p.n)) { p.rest_ran_lean(); return t; }
    p.take_flags(flag.data());
    p.release_crowds();
    p.collect_given_up_and_breaks();
    t.asked_sig = p.some_crowd_is_fresh();
    p.pick_leaders(t.asked_sig ? sig : NULL);
    if (!p.list_full.empty()) { t.round = true; return t; }
    if (!p.advance()) return t;
    t.asked_refs = p.level_break;
    if (p.level_break) p.carry_levels(refs);
    p.build_segments();
    t.round = true;
    return t;
}

/* the round decodes exactly the frames [lo, hi) with the lean kernel, as one range */
static void expect_lean_range(const ChainPlan &p, int lo, int hi)
{
    expect_list(p.list_lean, range(lo, hi), "lean list");
    expect(p.list_full.empty(), "no full list");
    expect(p.contiguous && !p.any_hard && p.run_lo == lo && p.run_hi == hi, "one lean range");
}

static void broken_links()
{
    const uint8_t moved = sdv::VF_BREAK | sdv::VF_MOVED, retuned = sdv::VF_BREAK | sdv::VF_RETUNED;
    {   /* Frames up to the first break are final; the frame behind a broken link is an anchor, the frames behind it are predicted from it and all of
         * them are decoded again, over the whole rest of the batch. */
        current = "one broken link";
        ChainPlan p; p.begin(10, 0, false);
        std::vector<uint8_t> flag(10, 0); flag[3] = moved;
        const Turn t = turn(p, flag, NULL, NULL);
        expect(t.round && !t.asked_sig && !t.asked_refs, "a round, nothing more read back");
        expect(p.first == 4, "first becomes 4");
        expect_list(p.anchors, { 4 }, "anchors");
        expect_list(p.first_of, { 4, 4, 4, 4, 4, 4 }, "first_of");
        expect_lean_range(p, 4, 10);
        expect(p.patches.empty(), "no patches");
        expect(p.any_moved, "the link broke over coordinates or histories: history carry wanted");
    }
    {   /* "the first of a run of broken links, that is": frames further into a run of links that moved are predicted from the run's first anchor. */
        current = "a run of moved links";
        ChainPlan p; p.begin(10, 0, false);
        std::vector<uint8_t> flag(10, 0); flag[3] = flag[4] = flag[5] = moved;
        const Turn t = turn(p, flag, NULL, NULL);
        expect(t.round && p.first == 4, "first becomes 4");
        expect_list(p.anchors, { 4 }, "anchors");
        expect_list(p.first_of, { 4, 4, 4, 4, 4, 4 }, "first_of");
        expect_lean_range(p, 4, 10);
        expect(p.any_moved, "history carry wanted");
    }
    {   /* "... unless the frame only came out with other levels" (VF_RETUNED without VF_MOVED): its successor is started from what it left, so every
         * frame behind such a link is an anchor of its own.  The reference levels are read back; with no frame handing on the level it got (refs: in 50,
         * out 60 + frame) nothing passes through and nothing is patched.  No link moved and no history is off: the history carry has nothing to do. */
        current = "a run of links that only re-tuned";
        ChainPlan p; p.begin(10, 0, false);
        std::vector<uint8_t> flag(10, 0); flag[3] = flag[4] = flag[5] = retuned;
        std::vector<uint8_t> refs(30, 0);
        for (int k = 0; k < 10; k++) { refs[3 * k] = 50; refs[3 * k + 1] = (uint8_t)(60 + k); refs[3 * k + 2] = 1; }
        const Turn t = turn(p, flag, NULL, refs.data());
        expect(t.round && t.asked_refs && p.first == 4, "a round behind frame 3, the levels read back");
        expect_list(p.anchors, { 4, 5, 6 }, "anchors");
        expect_list(p.first_of, { 4, 5, 6, 6, 6, 6 }, "first_of");
        expect_lean_range(p, 4, 10);
        expect(p.patches.empty(), "no patches");
        expect(!p.any_moved, "no history carry");
    }
    {   /* A level that passes through: frame 3 re-tuned and hands on 60 where it handed on 50 before.  Frame 4 (the anchor: the copy of its predecessor's
         * state brings the 60, no patch) went in with 50 and handed 50 on: it passes its level through, so 60 arrives at frame 5, whose link held - frame 5
         * is patched and decoded again as an anchor of its own; it passed 50 through too, so frame 6 gets the 60 as well; frame 6 went in with 50 and
         * handed on 55: there the carry ends, frame 7 is predicted from anchor 6 like the rest. */
        current = "a level carried along the chain";
        ChainPlan p; p.begin(10, 0, false);
        std::vector<uint8_t> flag(10, 0); flag[3] = retuned;
        std::vector<uint8_t> refs(30, 0);
        for (int k = 0; k < 10; k++) { refs[3 * k] = 50; refs[3 * k + 1] = 50; refs[3 * k + 2] = 1; }
        refs[3 * 3 + 1] = 60; refs[3 * 6 + 1] = 55;
        const Turn t = turn(p, flag, NULL, refs.data());
        expect(t.round && t.asked_refs && p.first == 4, "a round behind frame 3, the levels read back");
        expect(p.patches == std::vector<uint32_t>({ 5u | (60u << 24), 6u | (60u << 24) }), "frames 5 and 6 start from level 60");
        expect_list(p.anchors, { 4, 5, 6 }, "anchors");
        expect_list(p.first_of, { 4, 5, 6, 6, 6, 6 }, "first_of");
        expect_lean_range(p, 4, 10);
    }
}

static void crowds()
{
    const uint8_t gave_up = sdv::VF_ABORTED;
    struct Sigs { const char *name; int first_window, second_window; bool none; std::vector<int> leaders; };
    /* 20 frames give up side by side for the first time: a crowd, led by the first frame of every window it looks at - a frame whose line begins two
     * pixels or more beside its leader's.  Without signatures (0xFF, or none read) the crowd's first frame leads alone. */
    const Sigs cases[] = { { "a fresh crowd over two windows", 40, 46, false, { 10, 20 } }, { "a fresh crowd, a difference of one", 40, 41, false, { 10 } },
                           { "a fresh crowd, every signature 0xFF", 0xFF, 0xFF, false, { 10 } }, { "a fresh crowd without signatures", 40, 46, true, { 10 } } };
    for (const Sigs &c : cases) {
        current = c.name;
        ChainPlan p; p.begin(40, 0, false);
        std::vector<uint8_t> flag(40, 0), sig(40, 0xFF);
        for (int k = 10; k < 30; k++) { flag[k] = gave_up; sig[k] = (uint8_t)(k < 20 ? c.first_window : c.second_window); }
        const Turn t = turn(p, flag, c.none ? NULL : sig.data(), NULL);
        expect(t.round && t.asked_sig, "a round; the predicate asks for the signatures");
        expect_list(p.list_full, c.leaders, "full list");
        expect(p.list_lean.empty() && p.first == 0, "nothing else in the round, nothing final yet");
        for (int k = 10; k < 30; k++) {
            const bool leads = k == c.leaders[0] || (c.leaders.size() > 1 && k == c.leaders[1]);
            expect(p.hard[k] == (leads ? ChainPlan::H_FULL : ChainPlan::H_PENDING), "leaders H_FULL, the others H_PENDING");
        }
    }
    {   /* "a leader needs followers": the window changes right behind the crowd's first frame, but a frame leads only once its leader has two followers -
         * frames 11 and 12 stay with frame 10, frame 13 leads the rest. */
        current = "a leader needs two followers";
        ChainPlan p; p.begin(40, 0, false);
        std::vector<uint8_t> flag(40, 0), sig(40, 0xFF);
        for (int k = 10; k < 30; k++) { flag[k] = gave_up; sig[k] = k == 10 ? 40 : 46; }
        turn(p, flag, sig.data(), NULL);
        expect_list(p.list_full, { 10, 13 }, "full list");
    }
    {   /* fewer than 8 in a row: damaged frames, not a state that does not fit - each to the full kernel, and by the full kernel from then on */
        current = "a run of seven given-up frames is no crowd";
        ChainPlan p; p.begin(40, 0, false);
        std::vector<uint8_t> flag(40, 0);
        for (int k = 10; k < 17; k++) flag[k] = gave_up;
        const Turn t = turn(p, flag, NULL, NULL);
        expect(t.round && !t.asked_sig, "a round, no signatures asked for");
        expect_list(p.list_full, range(10, 17), "full list");
        for (int k = 10; k < 17; k++) expect(p.hard[k] == ChainPlan::H_FULL, "all seven H_FULL");
    }
    {   /* ... and a crowd is fresh only when ALL its frames gave up for the first time: seven of these ten have been with the full kernel before, so the
         * ten are damaged frames like the seven were, and no signatures are asked for */
        current = "a long run with frames that gave up before is no crowd";
        ChainPlan p; p.begin(40, 0, false);
        std::vector<uint8_t> flag(40, 0);
        for (int k = 10; k < 17; k++) flag[k] = gave_up;
        turn(p, flag, NULL, NULL);
        for (int k = 17; k < 20; k++) flag[k] = gave_up;
        const Turn t = turn(p, flag, NULL, NULL);
        expect(t.round && !t.asked_sig, "a round, no signatures asked for");
        expect_list(p.list_full, range(10, 20), "full list");
    }
    {   /* The crowd waits while its first frame is still owed a sweep (it came back from the full kernel as given up); once that frame is settled the
         * crowd is decoded again as if the link into it had broken: predicted from what the leader found, by the lean kernel once more. */
        current = "a held crowd";
        ChainPlan p; p.begin(40, 0, false);
        std::vector<uint8_t> flag(40, 0);
        for (int k = 10; k < 20; k++) flag[k] = gave_up;
        turn(p, flag, NULL, NULL);
        expect_list(p.list_full, { 10 }, "round 1: the leader alone");
        Turn t = turn(p, flag, NULL, NULL);             /* the leader came back given up, the others have not been decoded since */
        expect(t.round, "round 2");
        expect_list(p.list_full, { 10 }, "round 2: the leader again");
        expect(p.list_lean.empty() && !p.redo_first, "round 2: nothing else");
        for (int k = 11; k < 20; k++) expect(p.held[k] == 1 && p.hard[k] == ChainPlan::H_PENDING, "round 2: the crowd is held, still pending");
        flag[10] = 0;                                   /* the leader's sweeps are settled: it ran to its end and its link into frame 11 stands as it was */
        t = turn(p, flag, NULL, NULL);
        expect(t.round && p.first == 11, "round 3: the leader is final");
        expect_list(p.anchors, { 11 }, "round 3: anchors");
        expect_lean_range(p, 11, 40);
        for (int k = 11; k < 20; k++) expect(p.held[k] == 0 && p.hard[k] == ChainPlan::H_TRIED, "round 3: the crowd has its second try with the lean kernel");
    }
}

static void window_rule_and_verdict()
{
    {   /* A tape that plays: all links hold, nothing of the plan is touched but `slow`. */
        current = "a tape that plays";
        ChainPlan p; p.begin(20, 0, false);
        std::vector<uint8_t> flag(20, 0);
        const Turn t = turn(p, flag, NULL, NULL);
        expect(!t.round && p.first == 0 && p.kind.empty(), "no round, no working copy of the flags made");
    }
    {   /* Behind 24 repair rounds, with more than one link in 64 of the rest broken, the round decodes a window only: four times what the last round
         * settled, 16 frames at least.  400 frames, every 10th link breaks (moved), first at 9: each turn settles 10 frames.  Turns 1-24 decode the whole
         * rest; turn 25 advances first from 240 to 250 of 400 (15 breaks * 64 > 150) and decodes [250, 290). */
        current = "the window behind 24 repair rounds";
        ChainPlan p; p.begin(400, 0, false);
        std::vector<uint8_t> flag(400, 0);
        for (int k = 9; k < 399; k += 10) flag[k] = sdv::VF_BREAK | sdv::VF_MOVED;
        for (int r = 1; r <= 25; r++) {
            for (int k = 0; k < p.first; k++) flag[k] = 0;
            turn(p, flag, NULL, NULL);
            if (r == 24) expect(p.first == 240 && p.hi == 400, "round 24: still the whole rest");
        }
        expect(p.first == 250 && p.hi == 290, "round 25: a window of 40 frames");
        expect(p.first_of.size() == 40 && p.run_lo == 250 && p.run_hi == 290, "round 25: lists for the window only");
    }
    {   /* The worn-tape mark: most of the call's frames took lines through the general path; the cold first frame does not count, a call of fewer than 8
         * frames says nothing. */
        current = "the worn-tape mark";
        ChainPlan p; p.begin(13, 0, false);
        std::vector<uint8_t> flag(13, sdv::VF_BREAK | sdv::VF_MOVED | sdv::VF_SLOW);
        for (int k = 7; k < 13; k++) flag[k] = 0;
        p.take_flags(flag.data());              /* frames 0-6 of 13 slow */
        bool worn = false, plain = false; unsigned calls = 3;
        p.judge_tape(false, false, false, 0, 0, worn, plain, calls);
        expect(worn && !plain && calls == 0, "7 of 13: worn; no frame went to the full kernel: the plain build is not asked for");
        p.judge_tape(true, false, false, 0, 0, worn, plain, calls);
        expect(!worn, "6 of the 12 behind the cold frame: not worn");
        ChainPlan q; q.begin(7, 0, false);
        std::vector<uint8_t> all_slow(7, sdv::VF_BREAK | sdv::VF_SLOW);
        q.take_flags(all_slow.data());
        q.judge_tape(false, false, false, 0, 0, worn, plain, calls);
        expect(!worn, "a call of 7 frames, all slow, leaves the mark off");
        worn = true;
        ChainPlan r; r.begin(7, 0, false);
        r.judge_tape(false, false, false, 0, 0, worn, plain, calls);
        expect(worn, "a call of 7 frames, none slow, leaves the mark on");
    }
}

int main()
{
    broken_links();
    crowds();
    window_rule_and_verdict();
    if (failures) printf("%d expectations failed\n", failures); else printf("PLAN_OK\n");
    return failures;
}
