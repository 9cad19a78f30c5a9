/*
 * stc007_chain_plan.h - the host's decisions in the chain speculation of sdv_binarize_frames (stc007_frames_engine.inc): which frames of a call are
 * final, which are decoded again in the next round, by which kernel and from which state.  Plain host code on bytes the driver has read back: nothing in
 * here calls the runtime, so a program without a device can feed it flags by hand (tests/emu/stc007_plan_check.cpp).  Included behind stc007_device.h
 * (the VF_ values of the flag byte a frame leaves, v2d_store_state).
 *
 * A round of the driver's loop calls the steps in the order they stand here; what a step needs of the device arrives as a pointer to const bytes.
 */
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

struct ChainPlan {
    /* hard[k]: what the frame has been through */
    enum : uint8_t { H_NONE = 0, H_FULL = 1 /* full kernel from now on */, H_PENDING = 2 /* gave up in a crowd, waits for the crowd's first frame */,
                     H_TRIED = 3 /* ... and has had its second try with the lean kernel */, H_NEW = 0xFF /* given up for the first time, in this round */ };

    int n = 0;
    int first = 0;                  /* frames below are final */
    int repair_rounds = 0;
    /* per frame of the call */
    std::vector<uint8_t> kind;      /* how the frame left the chain (VF_KIND of its flag) as the steps below rewrite it: the plan's working copy of the read-back,
                                     * made by take_flags for [first, n) of the round.  advance and carry_levels also look at kind[first - 1] when a released
                                     * crowd leaves `first` where it was (redo_first): what an earlier round left there - VF_BREAK, since `first` only moves
                                     * to the frame behind a broken link - or VF_OK behind the cold chain's first frame, which was never taken (its link
                                     * is the copy of its outcome into frame 1, and frame 1 cannot be pending before `first` has moved) */
    std::vector<uint8_t> hard, held, is_anchor, changed, in_round;
    std::vector<uint8_t> slow;      /* the last decode of the frame took lines through the general path (VF_SLOW) */
    std::vector<uint8_t> hist_off;  /* the link behind the frame broke (also) over the 16-frame history (VF_HIST) */
    /* the round that is being planned */
    std::vector<int> list_lean, list_full, anchors, first_of;
    std::vector<uint32_t> patches;  /* frame | level << 24 (sdv_k_ref_patch) */
    bool redo_first = false;        /* the frame at `first` leads a released crowd: it is decoded again as if the link into it had broken */
    int n_break = 0, b0 = -1, n_leaders = 0;        /* broken links, the first of them, crowd leaders */
    bool fresh_crowd = false;       /* list_full holds a crowd whose frames all gave up for the first time (collect_given_up_and_breaks) */
    int hi = 0;                     /* the round decodes frames of [first, hi) */
    bool level_break = false;       /* a link of [first, hi) broke over the levels only: carry_levels has something to do (it wants the refs bytes) */
    bool any_moved = false;         /* a link broke over coordinates or histories: the history carry has something to do */
    bool any_hard = false, contiguous = true;       /* of the round's frames: some go to the full kernel; they are one range [run_lo, run_hi) */
    int run_lo = 0, run_hi = 0;

    /* A call of n frames whose frames below first_ are final already (the cold chain's first frame); worn: every frame starts on the full kernel. */
    void begin(int n_, int first_, bool worn)
    {
        n = n_; first = first_; repair_rounds = 0;
        hard.assign((size_t)n, worn ? (uint8_t)H_FULL : (uint8_t)H_NONE);
        held.assign((size_t)n, 0); is_anchor.assign((size_t)n, 0); changed.assign((size_t)n, 0); in_round.assign((size_t)n, 0);
        slow.assign((size_t)n, 0); hist_off.assign((size_t)n, 0);
        kind.clear();
    }

    /* 1. A tape that plays: every frame of [first, n) left the chain as predicted (all flags VF_OK) - nothing below has anything to do. */
    static bool all_links_hold(const uint8_t *flag, int first, int n)
    {
        uint64_t acc = 0; int k = first;
        for (; k + 8 <= n; k += 8) { uint64_t v; memcpy(&v, flag + k, 8); acc |= v; }
        for (; k < n; k++) acc |= flag[k];
        return acc == 0;
    }
    /* ... and none of them took a line through the general path */
    void rest_ran_lean() { std::fill(slow.begin() + first, slow.end(), (uint8_t)0); }

    /* 2. The flag bytes of [first, n) taken apart. */
    void take_flags(const uint8_t *flag)
    {
        kind.resize((size_t)n, (uint8_t)sdv::VF_OK);        /* (once per call, and not at all on a tape that plays) */
        for (int k = first; k < n; k++) {
            changed[(size_t)k] = (flag[k] & (sdv::VF_RETUNED | sdv::VF_MOVED)) == sdv::VF_RETUNED; slow[(size_t)k] = (flag[k] & sdv::VF_SLOW) ? 1 : 0;
            hist_off[(size_t)k] = (flag[k] & sdv::VF_HIST) ? 1 : 0;
            kind[(size_t)k] = flag[k] & sdv::VF_KIND;
        }
    }

    /* 3. A frame the lean kernel gave up is decoded by the full kernel, from the state it has, and by the full kernel from then on -
     * unless it gave up together with the frames behind it.  That is not a damaged frame but a state that does not fit any more
     * (the data window moved): the full kernel would search every one of those frames for the new window, where the reference
     * searches the first and hands the result on.  So only the first frame of such a crowd is decoded now; the others wait, and
     * are then predicted from what it found and given to the lean kernel once more.
     * Here the crowds whose first frame is settled are released, the others held.  Returns redo_first. */
    bool release_crowds()
    {
        list_lean.clear(); list_full.clear();
        redo_first = false;
        for (int k = first; k < n; k++) {
            held[(size_t)k] = 0;
            if (kind[(size_t)k] == sdv::VF_ABORTED && hard[(size_t)k] == H_PENDING) {       /* to be decoded again: as if the link into it had broken */
                /* ... once the frame in front of the crowd is settled: while that one is still owed a reference-level sweep (it came back from the full
                 * kernel as given up) its outcome is a guess, and the crowd goes on waiting */
                if (k > first && (held[(size_t)k - 1] || (kind[(size_t)k - 1] == sdv::VF_ABORTED && hard[(size_t)k - 1] != H_PENDING))) { held[(size_t)k] = 1; continue; }
                kind[(size_t)k] = sdv::VF_OK;
                if (k > first) kind[(size_t)k - 1] = sdv::VF_BREAK; else redo_first = true;
            }
        }
        return redo_first;
    }

    /* 4. Frames a lean wave gave up: all of them to the full kernel, each from the state it has (list_full; pick_leaders thins it out) - and whether
     * some run of them is a fresh crowd (8 or more in a row, all given up for the first time).  Broken links: counted, and the frames behind them marked
     * as anchors. */
    void collect_given_up_and_breaks()
    {
        n_break = 0; b0 = -1; n_leaders = 0;
        fresh_crowd = false;
        int run_len = 0; bool run_new = true;       /* the run of consecutive given-up frames that ends at the last entry of list_full */
        for (int k = first; k < n; k++) {
            if (held[(size_t)k]) continue;
            if (kind[(size_t)k] == sdv::VF_ABORTED) {
                hard[(size_t)k] = hard[(size_t)k] == H_NONE ? H_NEW : H_FULL;
                if (list_full.empty() || list_full.back() != k - 1) { fresh_crowd = fresh_crowd || (run_len >= 8 && run_new); run_len = 0; run_new = true; }
                run_len++; run_new = run_new && hard[(size_t)k] == H_NEW;
                list_full.push_back(k);
            }
            else if (kind[(size_t)k] == sdv::VF_BREAK) {
                /* A broken link makes the next frame an anchor - the first of a run of broken links, that is.  The frames further
                 * into the run were started from states that descend from one now known to be wrong, so what they handed over, and
                 * the breaks behind them, may only be a consequence of that: the data coordinates a frame inherits pass through it
                 * unchanged as long as its lines decode with them (a few pixels off still decodes), and the 16-frame coordinate
                 * history passes through by construction.  An anchor with such a state would hand it down the chain one frame per
                 * round; predicted again from the run's first anchor the frames follow a jump of the data window in one round. */
                const bool in_run = k > first ? kind[(size_t)k - 1] == sdv::VF_BREAK : redo_first;
                if (b0 < 0) b0 = k;
                n_break++;
                /* ... unless the frame only came out with other levels than the model makes of what it went in with (VF_RETUNED without VF_MOVED): a
                 * lost line makes the worker measure black and white again from the pixels that follow, whatever they were before, so the frame
                 * most likely leaves the same levels when it is decoded again from the right state - its successor is started from what it left.
                 * Frames that moved their coordinates or histories are different: those pass through the 9-line window, the damper and the 16-frame
                 * history, what a frame leaves does depend on what it got, and the model from the run's first anchor is the better guess.
                 * (Measured on 10 000 frames: a line lost in every frame 51 -> 12 ms; the same rule for frames that moved, 16 jumps: 18 -> 312 ms.
                 * Tried on top and dropped: working out the levels of a whole run byte by byte from which bytes each frame passed on and which it set
                 * in the last round - black and white are measured again to nearly the same values by every damaged frame and pass for handed on.) */
                if (k + 1 < n) is_anchor[(size_t)k + 1] = (in_run && !changed[(size_t)k]) ? 0 : 1;
            }
        }
        fresh_crowd = fresh_crowd || (run_len >= 8 && run_new);
    }

    /* 5. Who leads a crowd.  Of a run of given-up frames that is a crowd (8 or more in a row, all of them given up for the first time) only the leaders go
     * to the full kernel: the first frame of every WINDOW the crowd looks at, that is: a crowd that spans several jumps (all of them out of reach of the
     * state the frames were started from) would otherwise find its windows one per pair of rounds - leader, the frames predicted from it, the next stretch
     * gives up, its leader ...  The lean waves leave where the line they gave up on began (FrameArgs::sig); a frame whose line begins two pixels or
     * more beside its crowd leader's leads a crowd of its own.  A guess like any other: a leader too many is a frame through the general kernel too
     * many, a leader missed is found the old way.
     * some_crowd_is_fresh: pick_leaders has a use for the give-up signatures (the driver reads them back only then). */
    bool some_crowd_is_fresh() const { return fresh_crowd; }
    /* sig: a byte per frame of the call, 0xFF = none; NULL: no signatures, every crowd is led by its first frame */
    void pick_leaders(const uint8_t *sig)
    {
        size_t w = 0;
        for (size_t i = 0; i < list_full.size();) {
            size_t j = i + 1;
            while (j < list_full.size() && list_full[j] == list_full[j - 1] + 1) j++;
            const bool fresh = crowd_is_fresh(i, j);
            int lead_sig = -1, since_lead = 0;
            for (size_t q = i; q < j; q++) {
                const int k = list_full[q];
                bool leader = !fresh || q == i;
                if (!leader && sig) {
                    const int sg = sig[k];
                    /* (a leader needs followers: the last few frames of a run stay with the leader they have - they would go through the general kernel one by one anyway) */
                    if (sg != 0xFF && lead_sig >= 0 && (sg >= lead_sig + 2 || sg + 2 <= lead_sig) && since_lead >= 2) leader = true;
                }
                if (leader) { hard[(size_t)k] = H_FULL; list_full[w++] = k; if (fresh) { lead_sig = sig && sig[k] != 0xFF ? (int)sig[k] : -1; since_lead = 0; n_leaders++; } }
                else { hard[(size_t)k] = H_PENDING; since_lead++; }
            }
            i = j;
        }
        list_full.resize(w);
    }

    /* 6. Frames up to the first break are final.  Behind it: the first link of every run of broken links, of this round or an earlier
     * one, is an anchor (the next frame starts from its predecessor's real outcome), the frames in between are predicted from
     * their anchor, and every segment whose anchor changed is decoded again - all of them in one round, over the whole rest of
     * the batch: decoding a short window at a time would pay the rounds a disturbance takes once per window.
     * Returns false when the whole chain holds (nothing is advanced then). */
    bool advance()
    {
        if (redo_first) b0 = first - 1;
        if (b0 < 0 && !redo_first) return false;
        const int done = b0 + 1 - first;
        first = b0 + 1;
        /* ... unless the chain still breaks in many places after more rounds than the history is deep: then the model does not fit
         * this tape (heavy noise re-tunes the binarizer all the time) and decoding everything again every round is wasted work -
         * from there on only a window that grows with what the last round settled */
        hi = n;
        if (++repair_rounds > 24 && (long long)n_break * 64 > (long long)(n - first)) {
            long long w = 4ll * done; if (w < 16) w = 16;
            if (first + w < n) hi = (int)(first + w);
        }
        /* what the links of the round broke over (... or the frame only re-tuned its levels but its successor holds another history than the one it hands
         * on: the first frames behind a jump of the window each measure their levels anew and are anchors one by one; what they were started from the
         * round before is older than what their predecessors hand on now - without the carry the right history would reach them one frame per round) */
        any_moved = false; level_break = false;
        for (int j = first > 1 ? first : 1; j < hi && !any_moved; j++) any_moved = kind[(size_t)j - 1] == sdv::VF_BREAK && (!changed[(size_t)j - 1] || hist_off[(size_t)j - 1]);
        for (int j = first > 1 ? first : 1; j < hi && !level_break; j++) level_break = kind[(size_t)j - 1] == sdv::VF_BREAK && changed[(size_t)j - 1];
        patches.clear();
        return true;
    }

    /* 7. A level that passes through.  The reference level is sticky: a frame whose lines read with the level it inherits hands it on as it got it.
     * When a link broke over the levels only, the frame behind it now starts from another reference level - and if it handed on the old one
     * unchanged the last time, it will most likely hand on the new one, to a successor that was started from the old one and whose link held.
     * Decoding only the frame behind the break would find that out one frame per round (a sweep that settles on an odd level is followed by 25
     * such frames on the tape of SURVEY 8d C3: 77 rounds); so the new level is carried along the chain for as long as the frames are known to
     * pass their level through, those frames get it written into the state they start from (sdv_k_ref_patch, behind the anchor copies) and
     * are decoded in this round too.  A guess like every other state the rounds start frames from: the frames themselves say whether it held.
     * refs: per frame of the call the reference level it went in with, the one it handed on, whether it pushed one pair into the history (3 bytes). */
    void carry_levels(const uint8_t *refs)
    {
        int prop = -1;
        for (int j = first > 1 ? first : 1; j < hi; j++) {
            const bool broken = kind[(size_t)j - 1] == sdv::VF_BREAK;
            if ((broken && !changed[(size_t)j - 1]) || hard[(size_t)j] == H_PENDING) { prop = -1; continue; }      /* a frame that moved: the run model takes over */
            const int had = refs[3 * j], gave = refs[3 * j + 1], brought = refs[3 * (j - 1) + 1];
            int incoming;
            if (prop >= 0) incoming = prop;
            else if (broken) incoming = brought;
            else continue;                                      /* nothing new arrives at this frame */
            if (!broken) {
                if (incoming == had) { prop = -1; continue; }   /* the level it had anyway */
                patches.push_back((uint32_t)j | ((uint32_t)incoming << 24));
                kind[(size_t)j - 1] = sdv::VF_BREAK; is_anchor[(size_t)j] = 1;         /* decoded again, from its own (patched) state */
            } else if (incoming != brought) patches.push_back((uint32_t)j | ((uint32_t)incoming << 24));     /* (the anchor copy brings the predecessor's old level) */
            prop = (incoming != had && gave == had) ? incoming : -1;
        }
    }

    /* 8. Only the segments whose anchor gets a new state are decoded again; the others keep what they have. */
    void build_segments()
    {
        anchors.clear(); first_of.resize((size_t)(hi - first));
        int cur = first; bool dirty = true;
        any_hard = false; contiguous = true;
        run_lo = first; run_hi = first;
        for (int k = first; k < hi; k++) {
            if (k == first || is_anchor[(size_t)k]) {       /* anchors stay anchors: a link that held is not predicted over */
                cur = k; dirty = k == first || kind[(size_t)k - 1] == sdv::VF_BREAK;
                if (dirty) anchors.push_back(k);
            }
            first_of[(size_t)(k - first)] = dirty ? cur : k;
            in_round[(size_t)k] = dirty ? 1 : 0;
            if (dirty) {
                add_to_round(k);
                if (k != run_hi) contiguous = false;
                run_hi = k + 1;
            }
        }
    }

    /* 9. The frames of [first, hi) the history carry gave another start state (patched: a byte per frame of the call) are decoded in this round too.
     * Returns how many it added. */
    size_t add_carried(const uint8_t *patched)
    {
        size_t reached = 0;
        for (int k = first; k < hi; k++)
            if (patched[k] && !in_round[(size_t)k]) { add_to_round(k); contiguous = false; reached++; }
        return reached;
    }

    /* 10. What the call says about the tape, for the next call on the stream.  A worn tape: most frames of the call did take lines through the general path
     * - the next call starts its frames on the full kernel.  Decided on what the frames did (VF_SLOW of their last decode), not on where they were scheduled
     * (a worn call schedules every frame on the full kernel: judged by that, the mark never came off again, and a cold one-frame call was enough to set it);
     * the cold first frame does not count, and a call of a few frames says nothing either way.
     * memo_ready: the call sent frames to the full kernel; with_snapshots: ... to its build with the trajectory snapshots, whose meetings frames_met counts. */
    void judge_tape(bool cold, bool memo_ready, bool with_snapshots, uint32_t frames_general, uint32_t frames_met,
                    bool &worn_tape, bool &plain_general, unsigned &plain_calls) const
    {
        const int from = cold ? 1 : 0;
        size_t n_slow = 0;
        for (int k = from; k < n; k++) n_slow += slow[(size_t)k];
        if (n - from >= 8) worn_tape = n_slow * 2 > (size_t)(n - from);
        /* (which build of the general kernel the next call takes: sdv_engine::plain_general) */
        if (memo_ready && n - from >= 8) {
            if (with_snapshots) { plain_general = worn_tape && frames_general >= (uint32_t)n && (uint64_t)frames_met * 16u < (uint64_t)frames_general; plain_calls = 0; }
            else plain_calls++;
        } else if (!memo_ready) { plain_general = false; plain_calls = 0; }
    }

private:
    /* list_full[i, j) is a run of consecutive frames: a crowd whose frames all gave up for the first time */
    bool crowd_is_fresh(size_t i, size_t j) const
    {
        bool fresh = j - i >= 8;
        for (size_t q = i; q < j && fresh; q++) fresh = hard[(size_t)list_full[q]] == H_NEW;
        return fresh;
    }
    void add_to_round(int k)
    {
        if (hard[(size_t)k] == H_PENDING) hard[(size_t)k] = H_TRIED;
        (hard[(size_t)k] == H_FULL ? list_full : list_lean).push_back(k);
        any_hard = any_hard || hard[(size_t)k] == H_FULL;
    }
};
