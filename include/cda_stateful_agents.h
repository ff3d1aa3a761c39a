/*
 * cda_stateful_agents.h - rule-based opponents WITH MEMORY: trend follower (chartist / contrarian), value trader (fundamentalist), execution of a parent order.
 *
 * The sibling family of cda_scripted_agents.h, whose laws are pure functions of one view of the book NOW.  A law here also reads and writes
 * CDA_STATEFUL_WORDS int64 words of per-(market, slot) state, resident in device memory, and this header is the law: the device kernel
 * (csrc/cda_stateful.inc k_stateful_actions), the host entry point (cda_stateful_advance_host) and the Python specification (stateful.py) all
 * state these functions.  Plain C, host and device.  Integer arithmetic only: no float enters the state.
 *
 * The VIEW is cda_script_view as it is (vol[] is not read: the kernel never sums volume).  Prices are what the book stores - multiples of the
 * market's tick.  x = best_bid + best_ask (twice the mid) exists on a QUOTED step: both sides non-empty.
 *
 * THE STATE of one slot: word 0 is the header - low 32 bits last_t (the t_step of the last advance), high 32 bits the tag 1 + profile index
 * (0: never written); words 1 .. 3 belong to the law.
 *
 * ONE UPDATE RULE for every law, cda_stateful_advance(profile, profile index, view, keys, state):
 *   fresh  = view.t_step == 0, or tag == 0, or tag != 1 + profile index        -> words 1 .. 3 = 0, then the law's step on this view
 *   else if last_t == view.t_step                                              -> nothing changes (a second call at one step is idempotent)
 *   else                                                                       -> the law's step ONCE on this view (no catching up over skipped steps)
 *   then the header is written.
 * Every law's init is "zero the words, then take the step", so a law is one step function.  A market that resets itself inside the step kernel
 * restarts its slots' memory at its next t_step == 0; a slot re-pointed at another profile starts clean.  cda_stateful_decide reads the profile,
 * the view and the post-advance state, nothing else.
 *
 * TREND      words: 1 fast EMA, 2 slow EMA (of x << 16), 3 count of quoted steps seen.
 *   step:    unquoted - nothing.  quoted - count == 0: fast = slow = x << 16; else ema += floor((x << 16 - ema) / 2^shift) for each; count += 1.
 *   decide:  count <= warmup: pass.  d = direction * (fast - slow), thr = (2 * band_ticks * tick) << 16.
 *            d > thr: market buy (1) if pos < max_position, else pass.  d < -thr: market sell (5) if pos > -max_position, else pass.  Else pass.
 * VALUE      words: 1 the private value V in units of x, 2 the initialised flag, 3 unused (0).
 *   step:    not initialised - quoted: V = x, flag = 1; unquoted: nothing.  Initialised (every LATER step, quoted or not) - one draw w (below):
 *            (w & 0xffffffff) < p_move_q32: bit 32 clear -> V += 2 * tick; set -> V -= 2 * tick, and V < 2 * tick -> V = 2 * tick.
 *   decide:  not initialised: pass.  b = 2 * band_ticks * tick.  The buy test comes first and, where it holds, settles the step:
 *            best_ask != 0 and 2 * best_ask < V - b: market buy if pos < max_position, else pass.
 *            else best_bid != 0 and 2 * best_bid > V + b: market sell if pos > -max_position, else pass.  Else pass.
 * EXECUTION  words: 1 consecutive steps behind schedule, 2 and 3 unused (0).  max_position does NOT bind this law: the target is its inventory bound.
 *   due(t) = target * clamp(t - start_step, 0, duration) / duration, truncated toward zero in 64 bits; s = sign(target);
 *   behind = s * (due(t_step) - pos) > 0.
 *   step:    behind: word 1 += 1; else word 1 = 0.
 *   decide, in this order:  t_step < start_step: pass.  s * (target - pos) <= 0 (reached or overshot - it never reverses): pass.  Not behind: pass.
 *            word 1 <= patience: ONE resting order at the touch of the acquiring side (bid for a buy target): own_orders[side] == 0 -> limit
 *            (2 / 6, price 0, price_offset 1), else modify (3 / 7, the same price words).  Else a market order (1 / 5).
 * Every order carries the profile's size_mean / size_sigma; a pass is (0, 0.0, 0.0, 0, 1).
 */
#ifndef CDA_STATEFUL_AGENTS_H
#define CDA_STATEFUL_AGENTS_H

#include <stdint.h>
#include "cda_scripted_agents.h"

#define CDA_STATEFUL_TREND      1
#define CDA_STATEFUL_VALUE      2
#define CDA_STATEFUL_EXECUTION  3
#define CDA_STATEFUL_MAX_PROFILES 16
#define CDA_STATEFUL_WORDS      4        /* int64 per (market, slot): 32 bytes, 32-byte aligned */
#define CDA_STATEFUL_MAX_SHIFT  12       /* slow_shift's bound: an EMA over about 4096 steps */
#define CDA_STATEFUL_MAX_BAND   4096     /* band_ticks' bound: (2 * band_ticks * tick) << 16 then fits 64 bits for every int32 tick */

/* The value law's draws live in a domain of their own: cda_script_draw's construction under the 64 fraction bits of pi behind the mix
 * domain's (0x082efa98ec4e6c89), so a value trader, a taker and a label mix with equal keys never share a draw. */
#define CDA_STATEFUL_DOMAIN 0x082efa98ec4e6c89ULL

typedef struct cda_stateful_profile {    /* 64 bytes */
    int32_t  law;                        /* CDA_STATEFUL_* */
    float    size_mean;                  /* [-1, 1]: the action's size_mean of every order the law sends */
    float    size_sigma;                 /* [0, 1] */
    int32_t  max_position;               /* >= 0: the inventory cap of the trend and value laws */
    int32_t  fast_shift, slow_shift;     /* trend: 0 <= fast_shift < slow_shift <= 12 */
    int32_t  band_ticks;                 /* trend, value: 0 .. 4096 ticks of the MID the signal must clear */
    int32_t  direction;                  /* trend: +1 follows, -1 fades */
    int32_t  warmup;                     /* trend: >= 0, quoted steps seen before it trades: it passes while count <= warmup */
    int32_t  patience;                   /* execution: >= 0, steps behind schedule worked passively before it crosses */
    uint64_t p_move_q32;                 /* value: 0 .. 2^32, V moves when the 32-bit draw is below it (2^32 = every step) */
    int32_t  target;                     /* execution: != 0, the parent order in units of position (> 0 buys) */
    int32_t  start_step;                 /* execution: >= 0 */
    int32_t  duration;                   /* execution: >= 1 steps over which the schedule is linear */
    int32_t  pad0;
} cda_stateful_profile;

/* every bound of every law, whatever the profile's own law: a profile is one record, valid or not */
CDA_RA_FN int cda_stateful_profile_valid(const cda_stateful_profile* p) {
    if (p->law < CDA_STATEFUL_TREND || p->law > CDA_STATEFUL_EXECUTION) return 0;
    if (!(p->size_mean >= -1.0f && p->size_mean <= 1.0f) || !(p->size_sigma >= 0.0f && p->size_sigma <= 1.0f)) return 0;     /* (a NaN fails both) */
    if (p->max_position < 0) return 0;
    if (p->fast_shift < 0 || p->fast_shift >= p->slow_shift || p->slow_shift > CDA_STATEFUL_MAX_SHIFT) return 0;
    if (p->band_ticks < 0 || p->band_ticks > CDA_STATEFUL_MAX_BAND || (p->direction != 1 && p->direction != -1) || p->warmup < 0) return 0;
    if (p->p_move_q32 > 0x100000000ULL) return 0;
    return p->target != 0 && p->start_step >= 0 && p->duration >= 1 && p->patience >= 0;
}

CDA_RA_FN uint64_t cda_stateful_draw(uint64_t seed, uint64_t counter, uint64_t market, uint32_t draw, uint32_t agent) {
    const uint64_t h0 = cda_ra_mix((seed ^ CDA_STATEFUL_DOMAIN) + counter * 0x9e3779b97f4a7c15ULL + market * 0xd1342543de82ef95ULL);
    return cda_ra_mix(h0 + (((uint64_t)draw << 32) | (uint64_t)agent));
}

/* floor(d / 2^s) for either sign, without leaning on what >> does to a negative value (numpy's and Python's >> floor) */
CDA_RA_FN int64_t cda_stateful_floor_shift(int64_t d, int32_t s) {
    return d >= 0 ? (int64_t)((uint64_t)d >> s) : -(int64_t)(((uint64_t)(-d) + ((1ULL << s) - 1ULL)) >> s);
}

/* the execution law's schedule: is the slot behind it at this view? */
CDA_RA_FN int cda_stateful_exec_behind(const cda_stateful_profile* pf, const cda_script_view* v) {
    int64_t el = (int64_t)v->t_step - (int64_t)pf->start_step;
    if (el < 0) el = 0;
    if (el > (int64_t)pf->duration) el = (int64_t)pf->duration;
    const int64_t due = (int64_t)pf->target * el / (int64_t)pf->duration;       /* C's / truncates toward zero */
    const int64_t gap = due - (int64_t)v->net_position;
    return pf->target > 0 ? gap > 0 : gap < 0;
}

/* state: CDA_STATEFUL_WORDS words, read and written in place */
CDA_RA_FN void cda_stateful_advance(const cda_stateful_profile* pf, int32_t profile_index, const cda_script_view* v, uint64_t seed, uint64_t counter, uint64_t market,
                                    uint32_t draw, uint32_t agent, int64_t* state) {
    const uint64_t hdr = (uint64_t)state[0];
    const uint32_t tag = (uint32_t)(hdr >> 32), want = (uint32_t)profile_index + 1u;
    const int fresh = v->t_step == 0 || tag == 0u || tag != want;
    if (!fresh && (uint32_t)hdr == (uint32_t)v->t_step) return;
    int64_t w1 = fresh ? 0 : state[1], w2 = fresh ? 0 : state[2], w3 = fresh ? 0 : state[3];
    const int quoted = v->best_bid != 0 && v->best_ask != 0;
    const int64_t x = (int64_t)v->best_bid + (int64_t)v->best_ask;
    if (pf->law == CDA_STATEFUL_TREND) {
        if (quoted) {
            const int64_t y = (int64_t)((uint64_t)x << 16);
            if (w3 == 0) { w1 = y; w2 = y; }
            else { w1 += cda_stateful_floor_shift(y - w1, pf->fast_shift); w2 += cda_stateful_floor_shift(y - w2, pf->slow_shift); }
            w3 += 1;
        }
    } else if (pf->law == CDA_STATEFUL_VALUE) {
        if (w2 == 0) {
            if (quoted) { w1 = x; w2 = 1; }
        } else {
            const uint64_t w = cda_stateful_draw(seed, counter, market, draw, agent);
            if ((w & 0xffffffffULL) < pf->p_move_q32) {
                const int64_t step = 2 * (int64_t)v->tick;
                if (((w >> 32) & 1ULL) == 0ULL) w1 += step;
                else { w1 -= step; if (w1 < step) w1 = step; }
            }
        }
    } else if (pf->law == CDA_STATEFUL_EXECUTION) {
        w1 = cda_stateful_exec_behind(pf, v) ? w1 + 1 : 0;
    }
    state[0] = (int64_t)(((uint64_t)want << 32) | (uint64_t)(uint32_t)v->t_step);
    state[1] = w1; state[2] = w2; state[3] = w3;
}

CDA_RA_FN void cda_stateful_decide(const cda_stateful_profile* pf, const cda_script_view* v, const int64_t* state, int32_t* category, float* size_mean, float* size_sigma,
                                   int32_t* price, int32_t* price_offset) {
    int32_t cat = 0;
    const int32_t pos = v->net_position, cap = pf->max_position;
    if (pf->law == CDA_STATEFUL_TREND) {
        if (state[3] > (int64_t)pf->warmup) {
            const int64_t d = (int64_t)pf->direction * (state[1] - state[2]);
            const int64_t thr = (int64_t)((uint64_t)(2 * (int64_t)pf->band_ticks * (int64_t)v->tick) << 16);
            if (d > thr) { if (pos < cap) cat = 1; }
            else if (d < -thr) { if (pos > -cap) cat = 5; }
        }
    } else if (pf->law == CDA_STATEFUL_VALUE) {
        if (state[2] != 0) {
            const int64_t V = state[1], b = 2 * (int64_t)pf->band_ticks * (int64_t)v->tick;
            if (v->best_ask != 0 && 2 * (int64_t)v->best_ask < V - b) { if (pos < cap) cat = 1; }
            else if (v->best_bid != 0 && 2 * (int64_t)v->best_bid > V + b) { if (pos > -cap) cat = 5; }
        }
    } else if (pf->law == CDA_STATEFUL_EXECUTION) {
        const int buy = pf->target > 0;
        const int64_t left = (int64_t)pf->target - (int64_t)pos;
        if (v->t_step >= pf->start_step && (buy ? left > 0 : left < 0) && cda_stateful_exec_behind(pf, v)) {
            if (state[1] <= (int64_t)pf->patience) cat = ((buy ? v->own_orders[0] : v->own_orders[1]) == 0 ? 2 : 3) + (buy ? 0 : 4);
            else cat = buy ? 1 : 5;
        }
    }
    *category = cat; *price = 0; *price_offset = 1;
    *size_mean = cat ? pf->size_mean : 0.0f;
    *size_sigma = cat ? pf->size_sigma : 0.0f;
}

#endif
