// tip_measure.h — THE table of the measurement switches: one line per TIP_* environment variable the measurement build
// (-DTIP_MEASURE, `make measure`) reads.  tip_internal.h expands it into the fields of MeasureSwitches, tip_schedule.hip into the one
// place that reads the environment (measure_switches()); include/tip_hip_debug.h repeats the names for the scripts' authors, and
// tests/test_measure_switches_cpu.py holds the three lists together.  No include guard: every includer defines TIP_SWITCH first.
//
// TIP_SWITCH(environment name, field type, field, parsing rule, default, meaning).  The parsing rules (tip_schedule.hip):
//   sw_bool     unset: the default; else off exactly when the value starts with '0'
//   sw_int      unset: the default; else atoi
//   sw_not_old  unset: the default; else off exactly when the value is the word "old"
// A switch stays here while a script under tools/ or a test sets it; one whose experiment is closed leaves with the code only it reached.

// the schedule's A/B selections (tip_schedule.hip, tip_abi.hip)
TIP_SWITCH("TIP_AUTO_SPLIT", bool, split, sw_bool, true, "0: no whole rounds + remainder split (tools/auto_sweep.py)")
TIP_SWITCH("TIP_AUTO_MERGE", bool, merge, sw_bool, true, "0: the two parts of a split never share one recurrence + projection")
TIP_SWITCH("TIP_RNN_ROWS4", bool, rows4, sw_bool, true, "0: AUTO keeps the 16-window recurrence kernels (forward and training step)")
TIP_SWITCH("TIP_HEAD", bool, head_ksplit, sw_not_old, true, "old: the streaming output projection on head_gemm_kernel")
// in-kernel time stamps, read back through the tip_debug_read_* hooks
TIP_SWITCH("TIP_FUSEDH_TRACE", bool, fusedh_trace, sw_bool, false, "hybrid encoder, inference and training forward (tools/fh_trace.py)")
TIP_SWITCH("TIP_FUSED2_TRACE", bool, fused2_trace, sw_bool, false, "two-window encoder (tools/f2_trace.py)")
TIP_SWITCH("TIP_BWD_TRACE", bool, bwd_trace, sw_bool, false, "fused backward kernels (tools/bwd_trace.py)")
TIP_SWITCH("TIP_RNN_TRACE", bool, rnn_trace, sw_bool, false, "clustered recurrence hand-off (tools/rnn_trace.py)")
TIP_SWITCH("TIP_HEAD_TRACE", bool, head_trace, sw_bool, false, "register-resident output projection (tools/head_trace.py)")
TIP_SWITCH("TIP_FLOW_TRACE", bool, flow_trace, sw_bool, false, "one-launch few-stream form (tools/flow_trace.py)")
// recurrence
TIP_SWITCH("TIP_RNN_ABLATE", int, rnn_ablate, sw_int, 0, "rnn_rows4_kernel with parts removed, WRONG results (bits: tip_hip_debug.h; tools/rnn_trace.py)")
TIP_SWITCH("TIP_RNN_W4", int, rnn_w4, sw_int, -1, "four-window tiles on 0: eight-wave, 1: four-wave workgroups; -1: by shape (tools/rnn_ab.py)")
// few-stream plan
TIP_SWITCH("TIP_LAT_FLOW", int, lat_flow, sw_int, kFlowMaxBatch, "largest batch of the one-launch form; 0: launch chain always (tools/b1_chain.py)")
// training step
TIP_SWITCH("TIP_DW_GROUP", bool, dw_group, sw_bool, true, "0: one launch per weight gradient (tools/train_timeline.sh)")
