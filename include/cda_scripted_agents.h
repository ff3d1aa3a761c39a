/*
 * cda_scripted_agents.h - rule-based opponents: pass, noise taker, market maker, order-imbalance trader.
 *
 * The reference has no scripted opponent; it points at them: its callback comments describe the always-pass collapse as invisible from
 * returns, and train/helper/helper.py carries order-imbalance and mid-price helpers nothing calls.  Here a LAW is a pure function of a
 * small integer VIEW of one (market, agent) pair and, for the taker, of a counter-based draw (include/cda_random_agents.h's mixer under a
 * domain constant of its own).  The device kernel (csrc/cda_scripted.inc k_script_actions), the host entry point
 * (cda_scripted_decide_host) and the numpy specification (scripted.py) all state this one function.  Plain C, host and device.
 *
 * Units: prices are what the book stores - multiples of the market's tick_size (MktRow::tick_size; cda_order.price of a market whose tick
 * is 5 moves in steps of 5) - so "the spread exceeds one tick" is best_ask - best_bid > tick.
 *
 * The action a law emits is the env's Dict action (action_helper.py:126-138): category 0 pass, 1 market buy, 2 limit bid, 3 modify bid
 * (the reference moves the trader's oldest order of that side), 5 market sell, 6 limit ask, 7 modify ask; price = level code 0 (the side's
 * best level, or one tick off last_price where the side is empty); price_offset 1 = join that level, 2 = one tick inside it.
 */
#ifndef CDA_SCRIPTED_AGENTS_H
#define CDA_SCRIPTED_AGENTS_H

#include <stdint.h>
#include "cda_random_agents.h"

#define CDA_SCRIPT_PASS       1
#define CDA_SCRIPT_TAKER      2
#define CDA_SCRIPT_MAKER      3
#define CDA_SCRIPT_IMBALANCE  4
#define CDA_SCRIPT_MAX_PROFILES 16
#define CDA_SCRIPT_MAX_DEPTH    10       /* CDA_K_ROWS: the ladder a law may sum */

/* The taker's draws live in a domain of their own: the key's seed is XORed with this constant (the 64 fraction bits of pi after the
 * first 64, 0x13198a2e03707344), so a scripted slot and a random-module slot (cda_random_action) with equal seeds never share a draw. */
#define CDA_SCRIPT_DOMAIN 0x13198a2e03707344ULL

typedef struct cda_script_profile {      /* 64 bytes */
    int32_t  law;                        /* CDA_SCRIPT_* */
    float    size_mean;                  /* [-1, 1]: the action's size_mean of every order the law sends */
    float    size_sigma;                 /* [0, 1] */
    int32_t  max_position;               /* >= 0: the inventory cap */
    int32_t  skew_position;              /* 0 .. max_position: beyond it the maker quotes the reducing side only */
    int32_t  max_orders;                 /* >= 1: own resting orders per side before the maker modifies instead of placing */
    int32_t  depth_levels;               /* 1 .. 10: levels per side summed into view.vol */
    int32_t  imb_num, imb_den;           /* imb_num >= imb_den >= 1: the imbalance ratio that triggers */
    int32_t  pad0;
    uint64_t p_trade_q32;                /* 0 .. 2^32: the taker trades when its 32-bit draw is below it (2^32 = always) */
    int32_t  pad1[4];
} cda_script_profile;

typedef struct cda_script_view {         /* 56 bytes: what a law may read about (market, agent) */
    int32_t t_step, net_position, tick;
    int32_t best_bid, best_ask;          /* 0: that side is empty */
    int32_t own_orders[2];               /* cda_book_agents' `orders` of the agent, bids / asks */
    int32_t own_best[2];                 /* ... and `best_price` */
    int32_t pad;
    int64_t vol[2];                      /* volume of the first depth_levels levels of the bids / asks */
} cda_script_view;

CDA_RA_FN int cda_script_profile_valid(const cda_script_profile* p) {
    if (p->law < CDA_SCRIPT_PASS || p->law > CDA_SCRIPT_IMBALANCE) return 0;
    if (!(p->size_mean >= -1.0f && p->size_mean <= 1.0f) || !(p->size_sigma >= 0.0f && p->size_sigma <= 1.0f)) return 0;     /* (a NaN fails both) */
    if (p->max_position < 0 || p->skew_position < 0 || p->skew_position > p->max_position || p->max_orders < 1) return 0;
    if (p->depth_levels < 1 || p->depth_levels > CDA_SCRIPT_MAX_DEPTH || p->imb_den < 1 || p->imb_num < p->imb_den) return 0;
    return p->p_trade_q32 <= 0x100000000ULL;
}

CDA_RA_FN uint64_t cda_script_draw(uint64_t seed, uint64_t counter, uint64_t market, uint32_t draw, uint32_t agent) {
    const uint64_t h0 = cda_ra_mix((seed ^ CDA_SCRIPT_DOMAIN) + counter * 0x9e3779b97f4a7c15ULL + market * 0xd1342543de82ef95ULL);
    return cda_ra_mix(h0 + (((uint64_t)draw << 32) | (uint64_t)agent));
}

/* DAgger's mixing draw (csrc/cda_scripted_label.inc k_script_label, cda_label_mix_host): cda_script_draw's construction in a third domain (the next 64
 * fraction bits of pi, 0xa4093822299f31d0), so whether a label is played is independent of what a taker with the same seed draws.  The label replaces the
 * slot's action when the low 32 bits lie below mix_q32 (0 .. 2^32: 0 = never, 2^32 = always). */
#define CDA_SCRIPT_MIX_DOMAIN 0xa4093822299f31d0ULL

CDA_RA_FN uint64_t cda_script_mix_draw(uint64_t seed, uint64_t counter, uint64_t market, uint32_t draw, uint32_t agent) {
    const uint64_t h0 = cda_ra_mix((seed ^ CDA_SCRIPT_MIX_DOMAIN) + counter * 0x9e3779b97f4a7c15ULL + market * 0xd1342543de82ef95ULL);
    return cda_ra_mix(h0 + (((uint64_t)draw << 32) | (uint64_t)agent));
}

CDA_RA_FN void cda_scripted_decide(const cda_script_profile* pf, const cda_script_view* v, uint64_t seed, uint64_t counter, uint64_t market, uint32_t draw,
                                   uint32_t agent, int32_t* category, float* size_mean, float* size_sigma, int32_t* price, int32_t* price_offset) {
    int32_t cat = 0, off = 1;
    const int32_t pos = v->net_position, cap = pf->max_position;
    if (pf->law == CDA_SCRIPT_TAKER) {
        const uint64_t w = cda_script_draw(seed, counter, market, draw, agent);
        if ((w & 0xffffffffULL) < pf->p_trade_q32) {
            const int buy = ((w >> 32) & 1ULL) == 0ULL;
            if (buy ? pos < cap : pos > -cap) cat = buy ? 1 : 5;
        }
    } else if (pf->law == CDA_SCRIPT_MAKER) {
        if (pos > cap) cat = 5;
        else if (pos < -cap) cat = 1;
        else {
            const int side = pos > pf->skew_position ? 1 : (pos < -pf->skew_position ? 0 : (int)(((uint32_t)v->t_step + agent) & 1u));
            cat = ((side ? v->own_orders[1] : v->own_orders[0]) >= pf->max_orders ? 3 : 2) + 4 * side;
            const int32_t best = side ? v->best_ask : v->best_bid;
            if (v->best_bid != 0 && v->best_ask != 0 && v->best_ask - v->best_bid > v->tick && (side ? v->own_best[1] : v->own_best[0]) != best) off = 2;
        }
    } else if (pf->law == CDA_SCRIPT_IMBALANCE) {
        const int64_t B = v->vol[0], S = v->vol[1];
        if (B * (int64_t)pf->imb_den > S * (int64_t)pf->imb_num && pos < cap) cat = 1;
        else if (S * (int64_t)pf->imb_den > B * (int64_t)pf->imb_num && pos > -cap) cat = 5;
    }
    *category = cat; *price = 0; *price_offset = off;
    *size_mean = cat ? pf->size_mean : 0.0f;
    *size_sigma = cat ? pf->size_sigma : 0.0f;
}

#endif
