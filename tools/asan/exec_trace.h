// What exec_stubs.cpp records and exec_order_check.cpp replays: one entry per HIP event call
// and per launch the executor (csrc/exec.cpp) makes, in call order.
#pragma once
#include <cstdint>
#include <vector>

struct TraceMember {  // one record of a launch: its payload identity and its grouping key
    uint64_t id;
    int key;
};
struct TraceEntry {
    enum Type { GETDEVICE, CREATE, RECORD, WAIT, LAUNCH, GROUP } type;
    int stream;  // 1 main, 2 side, 3 side 2 (the handles the program passes); 0 none
    int event;   // in creation order from 0; -1 none
    int kind;    // LAUNCH: the record kind the called launcher serves
    bool failed;
    std::vector<TraceMember> members;  // LAUNCH: one, GROUP: the plans of the launch
};
extern std::vector<TraceEntry> g_trace;
extern int g_fail_at;    // the n-th launch from now (1-based) fails with ISG_ERR_HIP; 0: none
extern int g_group_max;  // isg_pwg_group_max()
void trace_print(const TraceEntry& e);  // one line on stdout
