// cda_cap_table.inc - the table of a book capacity's market-wave kernels: included at the end of the per-capacity includes of cda_hip.hip (behind cda_kernels.inc,
// cda_orders.inc and cda_schedule.inc), it defines  cda::CDA_CAPNS::kernels.  The host picks the table once from the env's capacity (cap_kernels, cda_hip.hip) and
// launches through it: nothing else names a capacity's namespace.
#ifndef CDA_CAP_TABLE
#define CDA_CAP_TABLE
namespace cda {
struct Launch { dim3 grid, block; size_t smem; hipStream_t stream; };
struct CapKernels {
    int (*lds_bytes_per_wave)(int agents, int n_hist);
    void (*reset)(uint8_t*, Params, const uint64_t*, const uint8_t*, float*, int, int, uint8_t*, int, int, FinCapture);
    // k_step / k_tstep and k_run_random / k_tape_run take an argument struct of their own namespace: a launch helper of one signature stands for each instance
    void (*step[2][2][2])(const Launch&, uint8_t* arena, const Params&, const StepArgs&, const TapeArgs&);      // [tape on][info tensors][episode tallies]
    void (*run_random[2][2])(const Launch&, uint8_t* arena, const Params&, const RunArgs&, const TapeArgs&);    // [tape on][episode tallies]
    void (*place_order)(uint8_t*, Params, int, int, int, int, int, int);
    void (*tape_place_order)(uint8_t*, Params, int, int, int, int, int, int, TapeArgs);
    void (*mark_to_mkt)(uint8_t*, Params, int);
    void (*raw_snapshot)(uint8_t*, Params, float*);
    void (*order_stream)(uint8_t*, Params, OrderStreamArgs);
    void (*tape_order_stream)(uint8_t*, Params, OrderStreamArgs, TapeArgs);
    void (*sched_orders)(uint8_t*, Params, SchedArgs, int, int);
    void (*tsched_orders)(uint8_t*, Params, SchedArgs, int, int, TapeArgs);
};
}
#endif
namespace cda { namespace CDA_CAPNS {
template <bool INFO, bool TALLY> static void launch_k_step(const Launch& l, uint8_t* arena, const Params& P, const StepArgs& S, const TapeArgs&) {
    hipLaunchKernelGGL((k_step<INFO, TALLY>), l.grid, l.block, l.smem, l.stream, StepKernArgs{arena, P, S});
}
// the trade tape is on: the instances that write it (the tape's block behind k_step's arguments; the tallies by the market's ST_EP_ON bit)
template <bool INFO> static void launch_k_tstep(const Launch& l, uint8_t* arena, const Params& P, const StepArgs& S, const TapeArgs& T) {
    hipLaunchKernelGGL((k_tstep<INFO>), l.grid, l.block, l.smem, l.stream, TStepKernArgs{{arena, P, S}, T});
}
template <bool TALLY> static void launch_k_run_random(const Launch& l, uint8_t* arena, const Params& P, const RunArgs& R, const TapeArgs&) {
    hipLaunchKernelGGL((k_run_random<TALLY>), l.grid, l.block, l.smem, l.stream, RunKernArgs{arena, P, R});
}
static void launch_k_tape_run(const Launch& l, uint8_t* arena, const Params& P, const RunArgs& R, const TapeArgs& T) {
    hipLaunchKernelGGL(k_tape_run, l.grid, l.block, l.smem, l.stream, TRunKernArgs{{arena, P, R}, T});
}
static int lds_per_wave(int agents, int n_hist) { return lds_bytes_per_wave(agents, n_hist); }
static const CapKernels kernels = {
    lds_per_wave,
    k_reset,
    {{{launch_k_step<false, false>, launch_k_step<false, true>}, {launch_k_step<true, false>, launch_k_step<true, true>}},
     {{launch_k_tstep<false>, launch_k_tstep<false>}, {launch_k_tstep<true>, launch_k_tstep<true>}}},
    {{launch_k_run_random<false>, launch_k_run_random<true>}, {launch_k_tape_run, launch_k_tape_run}},
    k_place_order, k_tape_place_order, k_mark_to_mkt, k_raw_snapshot,
    k_order_stream, k_tape_order_stream, k_sched_orders, k_tsched_orders,
};
} }  // namespace cda::CDA_CAPNS
