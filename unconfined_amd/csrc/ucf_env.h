// ucf_env.h -- every environment knob of the library, read once, in one place.  Depends on the C library only.
//
// None of them is part of the product interface: they are tuning and diagnostic switches of the tests and of tools/.
// "kernel": the knob changes which kernel instantiation runs; "cut": it changes only how the work is cut into launches,
// work items or buffers (bit-neutral: test_pipeline_knobs_do_not_change_results and its neighbours).  The measurements
// behind the defaults stay beside the code that uses them.
#pragma once
#include <stddef.h>
#include <stdlib.h>

struct ucf_env {
    // plan_transform (ucf_launch_plan.h), integrate_kernel of the fast flavour
    int nsplit;            // UCF_NSPLIT (0): force 1, 2, 4 or 8 parts per work item.  cut
    int tail_lsplit;       // UCF_TAIL_LSPLIT (-1 = built-in): log2 of the parts of a launch's last items; 0 turns the finer tail off.  cut
    int tail_items;        // UCF_TAIL_ITEMS (-1 = built-in, one round of resident waves): how many items that tail holds.  cut
    bool persist;          // UCF_PERSIST (on; off when it starts with '0'): persistent grid that draws work from a counter.  cut
    bool nzc2;             // UCF_NZC2 (on; '0' off): two-depth launches run the NZC = 2 instantiations.  kernel
    bool nofold;           // UCF_NOFOLD (on; '0' off): plans that fold no screen term run the NOFOLD instantiations.  kernel
    int fold_waves_rt;     // UCF_FOLD_WAVES_RT (0): force 4, 5 or 6 waves per SIMD in the folded water-table kernel.  kernel
    int unfold_waves_rt;   // UCF_UNFOLD_WAVES_RT (0): force 3 or 4 waves per SIMD in the unfolded water-table kernel.  kernel
    // plan_transform, finish_kernel and point_kernel
    int finish_part;       // UCF_FINISH_PART (0 = from the LDS footprint): 16 / 32 / 64 lanes per scratch part, epsilon table in LDS.  kernel
    int grid_slots;        // UCF_GRID_SLOTS (8192; <= 0 = default): workgroups per launch when the interval areas live in global scratch.  cut
    // host side (ucf_plan.cpp, ucf_drawdown.cpp, ucf_multi.cpp, ucf_debug.cpp)
    int z_chunk;           // UCF_Z_CHUNK (0 = from the LDS budget): depths per launch; the depth count selects NZC.  cut (kernel through nz)
    double fast_eta_max;   // UCF_FAST_ETA_MAX (0 = none): cap of the fast evaluators' range, the rest goes to the generic one.  cut of the abscissae
    bool guard;            // UCF_GUARD (off; on when set, non-empty and not starting with '0'): buffers end at a page end.  allocation only
    size_t table_bytes;    // UCF_TABLE_BYTES (256 MiB; <= 0 = default): abscissa table per chunk of a point list.  cut
    size_t state_bytes;    // UCF_STATE_BYTES (8 GiB; <= 0 = default): integration state per launch.  cut
    int batch_layout;      // UCF_BATCH_LAYOUT (3): 3 = long lists run lane = point, anything else lane = Laplace sample.  kernel (the lane layout)
    int multi_groups;      // UCF_MULTI_GROUPS (0): cut every device's plans of ucf_drawdown_multi into n groups.  cut
    int debug_reps;        // UCF_DEBUG_REPS (1; < 1 = 1): ucf_debug_stages runs its launch sequence n times.  repeats only
    bool trace_launches;   // UCF_TRACE_LAUNCHES (off; as UCF_GUARD): synchronise and name every kernel on stderr before it starts.  no
};

// all the parsing; get(name) returns the value or NULL
inline ucf_env ucf_env_read(const char* (*get)(const char*))
{
    const auto num = [&](const char* name, int unset) { const char* e = get(name); return e ? atoi(e) : unset; };
    const auto on_unless_0 = [&](const char* name) { const char* e = get(name); return !e || *e != '0'; };
    const auto off_unless_set = [&](const char* name) { const char* e = get(name); return e && *e && *e != '0'; };
    const auto bytes = [&](const char* name, size_t dflt) { const char* e = get(name); const long long v = e ? atoll(e) : 0; return v > 0 ? (size_t)v : dflt; };
    ucf_env v;
    v.nsplit = num("UCF_NSPLIT", 0);
    v.tail_lsplit = num("UCF_TAIL_LSPLIT", -1);
    v.tail_items = num("UCF_TAIL_ITEMS", -1);
    v.persist = on_unless_0("UCF_PERSIST");
    v.nzc2 = on_unless_0("UCF_NZC2");
    v.nofold = on_unless_0("UCF_NOFOLD");
    v.fold_waves_rt = num("UCF_FOLD_WAVES_RT", 0);
    v.unfold_waves_rt = num("UCF_UNFOLD_WAVES_RT", 0);
    v.finish_part = num("UCF_FINISH_PART", 0);
    v.grid_slots = num("UCF_GRID_SLOTS", 8192);
    if (v.grid_slots <= 0) v.grid_slots = 8192;
    v.z_chunk = num("UCF_Z_CHUNK", 0);
    { const char* e = get("UCF_FAST_ETA_MAX"); v.fast_eta_max = e ? atof(e) : 0.0; }
    v.guard = off_unless_set("UCF_GUARD");
    v.table_bytes = bytes("UCF_TABLE_BYTES", (size_t)256 << 20);
    v.state_bytes = bytes("UCF_STATE_BYTES", (size_t)8 << 30);
    v.batch_layout = num("UCF_BATCH_LAYOUT", 3);
    v.multi_groups = num("UCF_MULTI_GROUPS", 0);
    v.debug_reps = num("UCF_DEBUG_REPS", 1);
    if (v.debug_reps < 1) v.debug_reps = 1;
    v.trace_launches = off_unless_set("UCF_TRACE_LAUNCHES");
    return v;
}

// the process environment, read on first use (defined in ucf_api.cpp, the one place that reads it; internal to the library, not an exported symbol)
__attribute__((visibility("hidden"))) const ucf_env& ucf_env_get();
