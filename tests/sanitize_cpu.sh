#!/bin/bash
# AddressSanitizer + UBSan over everything that runs on the host: the oracle, the host build of the lane code
# (tests/hostsim) and the native table driver (csrc/mcq_tables.cpp, linked against stubs of the GPU entry points).
# GPU sanitizers are not available on this pool; this is the CPU build only.   usage: tests/sanitize_cpu.sh
set -e
R=$(cd "$(dirname "$0")/.." && pwd); T=${TMPDIR:-/tmp}/mcq_san; mkdir -p $T
F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -shared -fPIC"
python3 - "$R" "$T" <<'PY'
import re, sys
R, T = sys.argv[1:]
h = open(R + "/include/mcq.h").read()
decls = re.findall(r"MCQ_API\s+([\w\s\*]+?)\b(mcq_\w+)\s*\(([^;]*?)\)\s*;", h, re.S)
own = {"mcq_tables_create", "mcq_tables_destroy", "mcq_tables_begin", "mcq_tables_resume", "mcq_tables_run",
       "mcq_tables_stats", "mcq_tables_state", "mcq_last_error", "mcq_eval_batch", "mcq_destroy"}
out = ['#include "mcq.h"', '#include <string>', '#include <atomic>', '#include <stdlib.h>',
       'static thread_local std::string g_err;', 'static std::atomic<long> g_calls(-1);', 'extern "C" {',
       'const char *mcq_last_error(void) { return g_err.c_str(); }',
       'int mcq_tables_set_error(const char *m) { g_err = m; return MCQ_EINVAL; }',
       'mcq_ctx *mcq_ctx_clone(const mcq_ctx *c) { return (mcq_ctx *)c; }', 'void mcq_destroy(mcq_ctx *) {}',
       # a stand-in equity so that mcq_tables_run (helper thread, thread pool) can run without a GPU: the same
       # function of the query as _fake_equity in tests/test_table_driver.py
       # MCQ_STUB_FAIL_AFTER=k: the k-th call after the variable appeared fails like a device error (a lock-step dying
       # half way); unsetting it disarms the countdown
       'int mcq_eval_batch(mcq_ctx *, const mcq_query *q, size_t n, uint64_t, uint64_t, int, mcq_result *out) {',
       '    const char *fa = getenv("MCQ_STUB_FAIL_AFTER");',
       '    if (!fa) g_calls = -1;',
       '    else { long e = -1; g_calls.compare_exchange_strong(e, atol(fa));',
       '           if (g_calls.fetch_sub(1) == 1) { g_err = "stand-in device failure"; return MCQ_EDEVICE; } }',
       '    for (size_t i = 0; i < n; i++) { unsigned x = q[i].hole[0] * 131u + q[i].hole[1] * 31u + q[i].n_players * 13u + q[i].n_board * 3u;',
       '        for (unsigned k = 0; k < q[i].n_board; k++) x += q[i].board[k] * 7u;',
       '        mcq_result r = {}; r.runs = 100; r.win = x % 101u; out[i] = r; }',
       '    return 0; }']
for ret, name, args in decls:
    if name in own:
        continue
    ret = ret.strip()
    body = "" if ret == "void" else ("return 0;" if "*" in ret or ret in ("float", "size_t") or name == "mcq_device_count"
                                     else "return MCQ_EDEVICE;")
    out.append("%s %s(%s) { %s }" % (ret, name, " ".join(args.split()), body))
open(T + "/stub.cpp", "w").write("\n".join(out) + "\n}\n")
PY
gcc $F -o $T/libmcq_oracle.so $R/oracle/mcq_oracle.c -lpthread
g++ $F -std=c++17 -Wno-unknown-pragmas -pthread -o $T/libmcq_hostsim.so $R/tests/hostsim/hostsim.cpp
g++ $F -std=c++17 -Wno-unknown-pragmas -I$R/include -o $T/libmcq_san.so $T/stub.cpp $R/neuron_poker_amd/csrc/mcq_tables.cpp -lpthread
cd $R
LD_PRELOAD="$(gcc -print-file-name=libasan.so) $(gcc -print-file-name=libubsan.so)" ASAN_OPTIONS=detect_leaks=0 \
MCQ_ORACLE_SO=$T/libmcq_oracle.so MCQ_HOSTSIM_SO=$T/libmcq_hostsim.so MCQ_LIBRARY=$T/libmcq_san.so MCQ_SAN_STUB=1 \
python3 -m pytest tests/test_oracle_golden.py tests/test_lane_arithmetic_host.py tests/test_table_driver.py \
  tests/test_evaluator_exhaustive_host.py tests/test_hot_boards_host.py -x -q \
  -k "not three_players_on_the_turn and not every_hand_in_every_split" -p no:cacheprovider "$@"
# (of the evaluator's sweep only test_a_slice_under_threads: six chunks, 2.3 M of the 133.8 M hands, a REDUCED slice)
# ThreadSanitizer over the threaded sweep entries (hs_eval7_splits, mcqo_calc_score_batch), the same reduced slice
FT="-O1 -g -fsanitize=thread -fno-omit-frame-pointer -shared -fPIC"
gcc $FT -o $T/libmcq_oracle_tsan.so $R/oracle/mcq_oracle.c -lpthread
g++ $FT -std=c++17 -Wno-unknown-pragmas -pthread -o $T/libmcq_hostsim_tsan.so $R/tests/hostsim/hostsim.cpp
LD_PRELOAD="$(gcc -print-file-name=libtsan.so)" TSAN_OPTIONS="report_signal_unsafe=0 exitcode=66" \
MCQ_ORACLE_SO=$T/libmcq_oracle_tsan.so MCQ_HOSTSIM_SO=$T/libmcq_hostsim_tsan.so \
python3 -m pytest tests/test_evaluator_exhaustive_host.py -x -q -k "slice_under_threads" -p no:cacheprovider
# ThreadSanitizer over the driver's threads (helper thread of the two-stream schedule, thread pool)
g++ -O1 -g -fsanitize=thread -fno-omit-frame-pointer -shared -fPIC -std=c++17 -Wno-unknown-pragmas -I$R/include \
    -o $T/libmcq_tsan.so $T/stub.cpp $R/neuron_poker_amd/csrc/mcq_tables.cpp -lpthread
LD_PRELOAD="$(gcc -print-file-name=libtsan.so)" TSAN_OPTIONS="report_signal_unsafe=0 exitcode=66" \
MCQ_LIBRARY=$T/libmcq_tsan.so MCQ_SAN_STUB=1 python3 -m pytest tests/test_table_driver.py -x -q -k "stand_in or thread_count or half_way" -p no:cacheprovider
# ... and over the shard workers of the multi-GPU entry (csrc/mcq_worker.hpp: submit / wait / join as mcq_multi.cpp drives them)
g++ -O1 -g -fsanitize=thread -fno-omit-frame-pointer -std=c++17 -I$R/include -o $T/tsan_worker $R/tests/tsan_worker.cpp -lpthread
TSAN_OPTIONS="exitcode=66" $T/tsan_worker
# ... and over the in-flight guard of the entry points (csrc/mcq_busy.hpp)
g++ -O1 -g -fsanitize=thread -fno-omit-frame-pointer -std=c++17 -o $T/tsan_busy $R/tests/tsan_busy.cpp -lpthread
TSAN_OPTIONS="exitcode=66" $T/tsan_busy
