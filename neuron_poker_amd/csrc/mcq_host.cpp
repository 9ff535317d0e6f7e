// mcq_host.cpp -- the C ABI of include/mcq.h on top of the gfx950 kernels.
//
// Host responsibilities only: argument validation, staging of the 16-byte query / 104-byte result records,
// the MT19937 walk of the parity mode (mcq_replay.hpp) and kernel launches.  There is no CPU evaluation path:
// without a HIP device mcq_create fails and every other entry point needs a context.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <exception>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "mcq_ctx.hpp"
#include "mcq_device.hpp"
#include "mcq_exact_ext.hpp"
#include "mcq_exact_hero.hpp"
#include "mcq_exact_hero_pre.hpp"
#include "mcq_exact_matrix.hpp"
#include "mcq_exact_runout.hpp"
#include "mcq_internal.hpp"
#include "mcq_mt_blocks.hpp"
#include "mcq_ranges.hpp"
#include "mcq_replay.hpp"

namespace {

thread_local std::string g_err;

constexpr size_t kReplayChunkBytes = 256u << 20;  /* draw bytes staged per launch by the host walk (numpy-stream entry) */
/* 64-bit words of a result row: mcq_result, or mcq_result_ways (the *_ways entries).  The staging code below handles rows
 * as `rw` words; row i of a buffer starts rw * 8 * i bytes in. */
constexpr uint32_t kPlainWords = sizeof(mcq_result) / 8u, kWaysWords = sizeof(mcq_result_ways) / 8u;
static_assert(kPlainWords == 13u && kWaysWords == 22u && sizeof(mcq_result_ways) % 16u == 0u, "result rows");
constexpr uint32_t kSeatsWords = sizeof(mcq_result_seats) / 8u; /* per-seat rows: the extended general path and the all-in enumeration */
static_assert(kSeatsWords == 32u && sizeof(mcq_seat) == 24u, "per-seat rows");
inline mcq_result *row_at(void *rows, size_t i, uint32_t rw) { /* (the first 13 words of either row are an mcq_result) */
    return reinterpret_cast<mcq_result *>(static_cast<char *>(rows) + i * rw * 8u);
}

}  // namespace

int mcq_fail(int code, const char *what, const char *detail) {
    g_err = what;
    if (detail) {
        g_err += ": ";
        g_err += detail;
    }
    return code;
}

namespace {

/* is stream s being captured into a graph? (a failing query counts as "no") */
bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return st != hipStreamCaptureStatusNone;
}

/* The scheduling scratch of stream s, at least `bytes` large.  A new stream takes a free slot, else the least
 * recently used one (after making s wait for that slot's last reader).  Growing is not possible while s is being
 * captured (hipMalloc / hipFree inside a capture would break it): the call fails cleanly instead. */
int scratch_for(mcq_ctx *c, hipStream_t s, size_t bytes, bool capturing, mcq_ctx::Scratch **out) {
    mcq_ctx::Scratch *slot = nullptr;
    for (auto &sc : c->scratch)
        if (sc.used && sc.stream == s) { slot = &sc; break; }
    if (!slot) {
        for (int i = 1; i < mcq_ctx::kScratch && !slot; i++)
            if (!c->scratch[i].used) slot = &c->scratch[i];
        if (!slot) {
            for (int i = 1; i < mcq_ctx::kScratch; i++) {
                mcq_ctx::Scratch &sc = c->scratch[i];
                if (sc.pinned) continue;
                if (!slot || sc.last_use < slot->last_use) slot = &sc;
            }
            if (!slot) return mcq_fail(MCQ_EINVAL, "mcq: every scheduling scratch slot is pinned by a captured graph");
            if (capturing) {
                if (hipEventQuery(slot->done) != hipSuccess) {
                    (void)hipGetLastError();
                    return mcq_fail(MCQ_EINVAL, "mcq: no free scheduling scratch for a stream that is being captured");
                }
            } else {
                HIP_TRY(hipStreamWaitEvent(s, slot->done, 0));
            }
        }
        slot->stream = s;
        slot->used = true;
    }
    if (bytes > slot->prefix.cap) {
        if (capturing)
            return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device: the context's scratch would have to grow inside a stream "
                                        "capture; issue one call of at least this size on this stream before capturing");
        if (slot->done_recorded) HIP_TRY(hipEventSynchronize(slot->done)); /* its last reader may still be running */
        HIP_TRY(slot->prefix.reserve(bytes));
    }
    slot->last_use = ++c->scratch_clock;
    if (capturing) slot->pinned = true; /* the graph keeps reading this buffer whenever it is replayed */
    *out = slot;
    return MCQ_OK;
}

}  // namespace

int mcq_run_slice(mcq_ctx *c, int mode, const mcq_query *d_q, uint32_t n, mcq_result *d_res, uint64_t seed,
                  uint64_t first_qid, uint64_t total_tasks, const uint8_t *d_draws, const uint64_t *d_off, hipStream_t s,
                  bool timed, uint64_t max_tasks, uint32_t part, uint32_t n_parts, const uint32_t *mt_seed32,
                  const uint64_t *d_prefix_ready, const McqMtbLaunch *mtb, uint32_t row_words) {
    if (mode == MCQ_MODE_PHILOX && c->law == MCQ_LAW_UNIFORM) mode = MCQ_INTERNAL_MODE_UNIFORM;
    const bool ways = row_words == kWaysWords;
    if ((!ways && row_words != kPlainWords) || (ways && mtb)) return mcq_fail(MCQ_EINVAL, "mcq: internal: bad result row length");
    const bool capturing = stream_capturing(s);
    if (capturing || !c->timing) timed = false; /* events recorded inside a capture cannot be read back */
    mcq_ctx::Scratch *sc = nullptr;
    const uint64_t *d_prefix = d_prefix_ready;
    if (!d_prefix) {
        int rc = scratch_for(c, s, ((size_t)n + 3) * sizeof(uint64_t), capturing, &sc);
        if (rc) return rc;
        d_prefix = (const uint64_t *)sc->prefix.p;
        HIP_TRY(mcq_launch_prep(d_q, n, d_res, (uint64_t *)sc->prefix.p, part, n_parts, c->knobs.n_cu, c->knobs.split_max, s,
                                row_words));
    }
    const McqGeometry geo = mcq_plan_geometry(c->knobs, mode, total_tasks, true, max_tasks);
    uint32_t split = geo.split;
    if (mode == MCQ_MODE_REPLAY_MT19937 && split > 2) split = 2; /* the parity kernel's lanes take four iterations at a time */
    /* queries in HBM (the host has not seen them): up to 1024 of them may be a small batch -- the prep kernel
     * decides the cut and the evaluation kernel reads it; more queries are at least as many tasks: never cut */
    if (total_tasks == 0 && n <= 1024u) split = MCQ_SPLIT_FROM_PREP;
    /* timing: the events take the evaluation kernel's own begin / end timestamps (no marker packets around a short
     * kernel); in parity mode the timed region starts in front of the stream walk */
    const int slot = (int)(c->n_timed % mcq_ctx::kRing);
    hipEvent_t t0 = timed ? c->ev0[slot] : nullptr, t1 = timed ? c->ev1[slot] : nullptr;
    if (mt_seed32) {
        if (timed) HIP_TRY(hipEventRecord(t0, s));
        t0 = nullptr;
        if (mtb)
            HIP_TRY(mcq_launch_mt_blocks(d_q, n, *mt_seed32, mtb->d_blk_off, mtb->d_grp_off, mtb->max_blocks, mtb->d_raw, mtb->d_exits,
                                         mtb->d_entries, mtb->d_gword, mtb->d_gits, mtb->d_gentry, mtb->d_ovf,
                                         const_cast<uint8_t *>(d_draws), d_off, d_res, mtb->d_part, s));
        else
            HIP_TRY(mcq_launch_mt_parse(d_q, n, *mt_seed32, const_cast<uint8_t *>(d_draws), d_off, d_res,
                                        const_cast<uint32_t *>(reinterpret_cast<const uint32_t *>(d_prefix + n + 2)),
                                        c->knobs.n_cu, s, row_words));
    }
    HIP_TRY(mcq_launch_eval(mode, d_q, n, d_prefix, d_res, seed, first_qid, c->d_luts, d_draws, d_off, geo.grid, geo.block, split,
                            part, n_parts, s, t0, t1, geo.work_wpb, ways));
    if (timed) c->n_timed++;
    /* a caller's stream may run on while another stream's call takes over the scratch: mark its last reader.  The
     * context's own stream (slot 0) is synchronised by every host entry before it returns. */
    if (sc && !capturing && sc != &c->scratch[0]) {
        HIP_TRY(hipEventRecord(sc->done, s));
        sc->done_recorded = true;
    }
    return MCQ_OK;
}

uint32_t mcq_tasks_of(const mcq_query &q) { return q.runs / MCQ_TASK_ITERS + (q.runs % MCQ_TASK_ITERS != 0u ? 1u : 0u); }

int mcq_validate_queries(const mcq_query *q, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!mcq_query_valid(mcq_query_words(q[i]))) {
            char buf[160];
            snprintf(buf, sizeof buf,
                     "query %zu invalid (cards must be distinct ids < 52, n_board <= 5, 1 <= n_players <= 10)", i);
            return mcq_fail(MCQ_EINVAL, buf);
        }
    return MCQ_OK;
}

namespace {

inline uint32_t tasks_of(const mcq_query &q) { return mcq_tasks_of(q); }
inline int validate(const mcq_query *q, size_t n) { return mcq_validate_queries(q, n); }
}  // namespace

static int kernel_times_impl(mcq_ctx *c, float *ms, int max_n);
/* the completion flag of the calls that hand their rows over in pinned memory (defined with the small-batch paths below) */
static int flag_ready(mcq_ctx *c);
static uint32_t next_ticket(mcq_ctx *c);
static int wait_ticket(mcq_ctx *c, uint32_t ticket, bool *by_flag, double est_us = 0.0);

namespace {

/* parity mode, independent streams: query i replays np.random.seed((seed + first_qid + i) mod 2^32).  The stream walk
 * runs on the DEVICE (mcq_mt_parse_kernel, one wave per query) and fills the draw buffer the evaluation kernel
 * reads; the host only lays the buffer out.  Chunks of queries whose draws fit c->replay_device_bytes. */
/* Few long queries (at most kMtbQueries in a chunk, at least kMtbMinBlocks state blocks among them) are parsed with
 * their state blocks side by side (mcq_mt_blocks.hpp): one 100 000-run query 6.5 -> 1.x ms.  The blocks a query needs are
 * an estimate with a margin; a query whose stream runs past them comes back with passes = UINT64_MAX and the call is
 * repeated with the serial walk. */
constexpr size_t kMtbQueries = 64;
constexpr uint64_t kMtbMinBlocks = 64, kMtbMaxBlocks = 1u << 18; /* (2.7 KB of scratch per block) */
int replay_batch_device(mcq_ctx *c, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id, void *out,
                        uint32_t rw, bool allow_blocks = true) {
    if (rw != kPlainWords) allow_blocks = false; /* the block-parallel walk writes 13-word rows only: the serial walk serves */
    HIP_TRY(c->h_off.reserve(n * sizeof(uint64_t)));
    HIP_TRY(c->d_off.reserve(n * sizeof(uint64_t)));
    uint64_t *off = (uint64_t *)c->h_off.p;
    struct Chunk { size_t a, b; uint64_t bytes, tasks, max_tasks; };
    std::vector<Chunk> chunks;
    size_t a = 0;
    uint64_t largest = 0;
    while (a < n) {
        Chunk ch = {a, a, 0, 0, 0};
        while (ch.b < n && ch.b - ch.a < 0x7fffffffu) {
            const uint64_t stride = ((uint64_t)q[ch.b].runs + 63u) & ~63ull;
            const uint64_t need = stride * mcq_draws_per_iteration(q[ch.b]);
            if (ch.b > ch.a && ch.bytes + need > c->replay_device_bytes) break;
            off[ch.b] = ch.bytes;
            ch.bytes += need;
            const uint64_t t = tasks_of(q[ch.b]);
            ch.tasks += t;
            if (t > ch.max_tasks) ch.max_tasks = t;
            ch.b++;
        }
        if (ch.bytes > largest) largest = ch.bytes;
        chunks.push_back(ch);
        a = ch.b;
    }
    HIP_TRY(c->d_draws.reserve(largest + 64));
    HIP_TRY(hipMemcpyAsync(c->d_off.p, off, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    const uint64_t timed0 = c->n_timed;
    bool by_blocks = false;
    for (const Chunk &ch : chunks) { /* stream order keeps a chunk's parse behind the previous chunk's evaluation */
        const uint32_t seed32 = (uint32_t)(seed + first_query_id + ch.a);
        const size_t m = ch.b - ch.a;
        McqMtbLaunch mtb = {};
        if (allow_blocks && c->mt_blocks && m <= kMtbQueries && chunks.size() == 1) {
            HIP_TRY(c->h_misc.reserve(2 * (m + 1) * sizeof(uint32_t)));
            uint32_t *blk = (uint32_t *)c->h_misc.p, *grp = blk + m + 1; /* block / group offsets of the queries */
            uint64_t total = 0, groups = 0, jumps = 0;
            for (size_t i = 0; i < m; i++) {
                const mcq_query &qq = q[ch.a + i];
                blk[i] = (uint32_t)total;
                grp[i] = (uint32_t)groups;
                const uint32_t n_opp = qq.n_players - 1u, n_deal = 5u - qq.n_board;
                if (qq.n_players >= 1 && qq.n_players <= 10 && qq.n_board <= 5 && 2u * n_opp + n_deal != 0u && qq.runs != 0u) {
                    const uint32_t nb = mcq_mtb_blocks_needed(50u - qq.n_board, n_opp, n_deal, qq.runs, c->mt_blocks_margin);
                    total += nb;
                    groups += (nb + MCQ_MTB_GROUP - 1u) / MCQ_MTB_GROUP;
                    if (nb > mtb.max_blocks) mtb.max_blocks = nb;
                    jumps += (nb - 1u) / MCQ_MTB_SEG;
                }
            }
            blk[m] = (uint32_t)total;
            grp[m] = (uint32_t)groups;
            const auto pad16 = [](uint64_t x) { return (x + 15u) & ~15ull; };
            /* segments side by side pay when the jumps (6.2 M word-XORs each: eight work-groups for 15 us, i.e. 0.4 us of
             * the whole GPU) and the three launches per round of 4096 blocks cost less than the longest query's blocks one
             * behind the other (0.19 us each) -- measured: ONE 6-max 100 000-run query 0.99 -> 0.29 ms; 64 queries of 780
             * blocks, all jumping: 1.18 -> 1.34 ms with the first jump kernel (49 us per 30 jumps) */
            const uint64_t rounds = (mtb.max_blocks + MCQ_MTB_SEG * MCQ_MTB_MAX_SEG - 1u) / (MCQ_MTB_SEG * MCQ_MTB_MAX_SEG);
            const bool use_jump = c->mt_jump && mtb.max_blocks > MCQ_MTB_SEG &&
                                  (c->mt_jump_always || 45.0 * (double)rounds + 0.4 * (double)jumps < 0.19 * (double)mtb.max_blocks);
            const uint64_t o_ovf = pad16(2 * (m + 1) * 4), o_ent = o_ovf + pad16(m * 4),
                           o_gen = o_ent + pad16(total * sizeof(McqMtbEntry)), o_gw = o_gen + pad16(groups * sizeof(McqMtbEntry)),
                           o_gi = o_gw + groups * MCQ_MTB_LANES * 4u, o_ex = o_gi + groups * MCQ_MTB_LANES * 4u,
                           o_raw = o_ex + total * MCQ_MTB_LANES * 4u, o_part = pad16(o_raw + total * MCQ_MT_N * 4u),
                           /* (the segments' start states by jump-ahead: only a query of more than one segment has any) */
                           part_bytes = use_jump ? m * mcq_mtb_part_words() * 4u : 0u,
                           bytes = o_part + part_bytes + 64u;
            bool room = total >= kMtbMinBlocks && total <= kMtbMaxBlocks;
            if (room && c->d_mt.reserve(bytes) != hipSuccess) { /* no room for the blocks' scratch (2.7 KB per block): the
                                                                  * serial walk, which needs none, serves the call */
                (void)hipGetLastError();
                room = false;
            }
            if (room) {
                char *base = (char *)c->d_mt.p;
                HIP_TRY(hipMemcpyAsync(base, blk, 2 * (m + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
                mtb.d_blk_off = (const uint32_t *)base;
                mtb.d_grp_off = mtb.d_blk_off + m + 1;
                mtb.d_ovf = (uint32_t *)(base + o_ovf);
                mtb.d_entries = base + o_ent;
                mtb.d_gentry = base + o_gen;
                mtb.d_gword = (uint32_t *)(base + o_gw);
                mtb.d_gits = (uint32_t *)(base + o_gi);
                mtb.d_exits = (uint32_t *)(base + o_ex);
                mtb.d_raw = (uint32_t *)(base + o_raw);
                mtb.d_part = use_jump ? (uint32_t *)(base + o_part) : nullptr;
                by_blocks = true;
            }
        }
        int rc = mcq_run_slice(c, MCQ_MODE_REPLAY_MT19937, (const mcq_query *)c->d_q.p + ch.a, (uint32_t)m,
                               row_at(c->d_res.p, ch.a, rw), seed, first_query_id + ch.a, ch.tasks ? ch.tasks : 1,
                               (const uint8_t *)c->d_draws.p, (const uint64_t *)c->d_off.p + ch.a, c->stream, true,
                               ch.max_tasks, 0, 1, &seed32, nullptr, mtb.d_blk_off ? &mtb : nullptr, rw);
        if (rc) return rc;
    }
    if (by_blocks && n <= c->publish_max_rows) {
        /* few long queries are a call of a quarter of a millisecond: the rows come back through pinned memory behind the
         * completion flag, as the small production calls' do (no copy, no stream synchronisation: 24 us against 7.5) */
        int rc = flag_ready(c);
        if (rc) return rc;
        const uint32_t ticket = next_ticket(c);
        HIP_TRY(mcq_launch_publish((mcq_result *)c->d_res.p, (mcq_result *)c->h_res.dev, n + (n & 1u), (uint32_t *)c->d_done.p,
                                   (uint32_t *)c->h_flag.dev, ticket, c->stream));
        rc = wait_ticket(c, ticket, nullptr, 0.0);
        if (rc) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(c->h_res.p, c->d_res.p, n * rw * 8u, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (by_blocks) { /* a stream that ran past its estimated blocks (never seen; the margin is eight blocks): the serial walk */
        const mcq_result *hr = (const mcq_result *)c->h_res.p;
        for (size_t i = 0; i < n; i++)
            if (hr[i].passes == ~0ull) return replay_batch_device(c, q, n, seed, first_query_id, out, rw, false);
    }
    memcpy(out, c->h_res.p, n * rw * 8u);
    float total = 0.f;
    const int launched = (int)(c->n_timed - timed0);
    if (launched > 0 && launched <= mcq_ctx::kRing) {
        float ms[mcq_ctx::kRing];
        if (kernel_times_impl(c, ms, launched) == launched)
            for (int i = 0; i < launched; i++) total += ms[i];
    }
    c->last_ms = total;
    return MCQ_OK;
}

/* parity mode coupled to ONE MT19937 stream that all queries continue in order, as consecutive reference calls
 * share numpy's global state (mcq_eval_batch_numpy_stream): a serial walk by construction, done on the host
 * (mcq_replay.hpp); chunks of queries whose draw bytes fit the staging budget. */
int replay_batch(mcq_ctx *c, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id, McqMt19937 *stream,
                 mcq_result *out, uint32_t rw = kPlainWords) {
    if (!stream) return replay_batch_device(c, q, n, seed, first_query_id, out, rw);
    if (rw != kPlainWords) return mcq_fail(MCQ_EINVAL, "mcq: internal: the numpy-stream walk writes mcq_result rows");
    std::vector<uint64_t> passes(n, 0);
    float replay_ms = 0.f;
    size_t a = 0;
    while (a < n) {
        size_t b = a;
        uint64_t bytes = 0, tasks = 0, max_tasks = 0;
        HIP_TRY(c->h_off.reserve((n - a < 65536 ? n - a : 65536) * sizeof(uint64_t)));
        uint64_t *off = (uint64_t *)c->h_off.p;
        while (b < n && b - a < 65536) {
            uint64_t stride = ((uint64_t)q[b].runs + 63u) & ~63ull;
            uint64_t need = stride * mcq_draws_per_iteration(q[b]);
            if (b > a && bytes + need > kReplayChunkBytes) break;
            off[b - a] = bytes;
            bytes += need;
            tasks += tasks_of(q[b]);
            if (tasks_of(q[b]) > max_tasks) max_tasks = tasks_of(q[b]);
            b++;
        }
        const size_t m = b - a;
        HIP_TRY(c->h_draws.reserve(bytes + 64));
        HIP_TRY(c->d_draws.reserve(bytes + 64));
        HIP_TRY(c->d_off.reserve(m * sizeof(uint64_t)));
        uint8_t *hd = (uint8_t *)c->h_draws.p;
        for (size_t i = 0; i < m; i++) {
            const mcq_query &qq = q[a + i];
            uint64_t stride = ((uint64_t)qq.runs + 63u) & ~63ull;
            passes[a + i] = mcq_replay_parse_stream(qq, *stream, hd + off[i], stride);
        }
        HIP_TRY(hipMemcpyAsync(c->d_draws.p, hd, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_off.p, off, m * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        int rc = mcq_run_slice(c, MCQ_MODE_REPLAY_MT19937, (const mcq_query *)c->d_q.p + a, (uint32_t)m,
                               (mcq_result *)c->d_res.p + a, seed, first_query_id + a, tasks, (const uint8_t *)c->d_draws.p,
                               (const uint64_t *)c->d_off.p, c->stream, true, max_tasks);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream)); /* staging buffers are reused by the next chunk */
        float ms = 0.f;
        if (c->timing && kernel_times_impl(c, &ms, 1) == 1) replay_ms += ms;
        a = b;
    }
    HIP_TRY(hipMemcpyAsync(c->h_res.p, c->d_res.p, n * sizeof(mcq_result), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(out, c->h_res.p, n * sizeof(mcq_result));
    for (size_t i = 0; i < n; i++) out[i].passes = passes[i];
    c->last_ms = replay_ms;
    return MCQ_OK;
}

/* validation + query upload shared by the host entry points (the caller has selected the context's device) */
int stage_queries(mcq_ctx *c, const mcq_query *q, size_t n, const void *out, const char *who, uint32_t rw = kPlainWords) {
    if (!c) return mcq_fail(MCQ_EINVAL, who, "null context");
    if (!q || !out) return mcq_fail(MCQ_EINVAL, who, "null buffer");
    if (n > 0x7fffffffu) return mcq_fail(MCQ_EINVAL, who, "n too large");
    int rc = validate(q, n);
    if (rc) return rc;
    uint64_t total_tasks = 0;
    for (size_t i = 0; i < n; i++) total_tasks += tasks_of(q[i]);
    if (total_tasks > 0xfffffff0ull) return mcq_fail(MCQ_EINVAL, who, "too many iterations in one call");
    HIP_TRY(c->h_q.reserve(n * sizeof(mcq_query)));
    HIP_TRY(c->h_res.reserve((n + (n & 1u)) * rw * 8u)); /* (whole 16-byte words: mcq_publish_kernel) */
    HIP_TRY(c->d_q.reserve(n * sizeof(mcq_query)));
    HIP_TRY(c->d_res.reserve((n + (n & 1u)) * rw * 8u));
    c->res_clean = 0; /* these entries zero their rows in the prep kernel and leave them filled */
    memcpy(c->h_q.p, q, n * sizeof(mcq_query));
    HIP_TRY(hipMemcpyAsync(c->d_q.p, c->h_q.p, n * sizeof(mcq_query), hipMemcpyHostToDevice, c->stream));
    c->last_ms = 0.f;
    return MCQ_OK;
}

}  // namespace

extern "C" {

const char *mcq_last_error(void) { return g_err.c_str(); }

int mcq_tables_set_error(const char *msg) { return mcq_fail(MCQ_EINVAL, msg); } /* for mcq_tables.cpp; not exported */

/* a second context like c (same device, dealing law and tuning) with its own stream and buffers; not exported */
mcq_ctx *mcq_ctx_clone(const mcq_ctx *c) {
    mcq_ctx *d = mcq_create(c->device, 0);
    if (d) {
        d->law = c->law;
        d->knobs = c->knobs; /* (the same device: the same CUs and occupancy) */
        d->direct_max_tasks = c->direct_max_tasks;
        d->direct_poll = c->direct_poll;
        d->direct_sleep = c->direct_sleep;
        d->direct_uniform_min = c->direct_uniform_min;
        d->ext_small = c->ext_small;
        d->mt_blocks = c->mt_blocks;
        d->mt_blocks_margin = c->mt_blocks_margin;
        d->mt_jump = c->mt_jump;
        d->mt_jump_always = c->mt_jump_always;
        d->publish_max_rows = c->publish_max_rows;
        d->timing = c->timing;
        d->replay_device_bytes = c->replay_device_bytes;
    }
    return d;
}

void mcq_version(int *major, int *minor, int *patch) {
    if (major) *major = MCQ_VERSION_MAJOR;
    if (minor) *minor = MCQ_VERSION_MINOR;
    if (patch) *patch = MCQ_VERSION_PATCH;
}

int mcq_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return mcq_fail(MCQ_EDEVICE, "hipGetDeviceCount", hipGetErrorString(e));
    return n;
}

void mcq_destroy(mcq_ctx *c) {
    if (!c) return;
    McqDeviceScope dev_(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    DevBuf *db[] = {&c->d_q, &c->d_res, &c->d_draws, &c->d_off, &c->d_ext,
                    &c->d_mt, &c->d_lists, &c->d_cnts};
    for (auto &sc : c->scratch) {
        sc.prefix.release();
        if (sc.done) (void)hipEventDestroy(sc.done);
    }
    for (DevBuf *b : db) b->release();
    PinBuf *pb[] = {&c->h_q, &c->h_res, &c->h_draws, &c->h_off, &c->h_misc, &c->h_flag};
    c->d_done.release();
    c->d_done_dev.release();
    for (PinBuf *b : pb) b->release();
    if (c->d_luts) (void)hipFree(c->d_luts);
    for (int i = 0; i < mcq_ctx::kRing; i++) {
        if (c->ev0[i]) (void)hipEventDestroy(c->ev0[i]);
        if (c->ev1[i]) (void)hipEventDestroy(c->ev1[i]);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

mcq_ctx *mcq_create(int device, int flags) {
    if (flags != 0) { mcq_fail(MCQ_EINVAL, "mcq_create: flags must be 0"); return nullptr; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        mcq_fail(MCQ_EDEVICE, "mcq_create: no HIP device available (this library has no CPU path)",
             e != hipSuccess ? hipGetErrorString(e) : nullptr);
        return nullptr;
    }
    if (device < 0 || device >= n) { mcq_fail(MCQ_EINVAL, "mcq_create: device ordinal out of range"); return nullptr; }
    mcq_ctx *c = new (std::nothrow) mcq_ctx();
    if (!c) { mcq_fail(MCQ_ENOMEM, "mcq_create: out of host memory"); return nullptr; }
    c->device = device;
    hipDeviceProp_t prop;
    McqTables *tabs = new (std::nothrow) McqTables();
    if (!tabs) { mcq_fail(MCQ_ENOMEM, "mcq_create: out of host memory"); delete c; return nullptr; }
    mcq_fill_tables(tabs);
#define CREATE_TRY(expr)                                                      \
    do {                                                                      \
        hipError_t e2_ = (expr);                                              \
        if (e2_ != hipSuccess) {                                              \
            mcq_fail(MCQ_EDEVICE, #expr, hipGetErrorString(e2_));                 \
            mcq_destroy(c);                                                   \
            delete tabs;                                                      \
            if (prev_dev >= 0) (void)hipSetDevice(prev_dev);                  \
            return nullptr;                                                   \
        }                                                                     \
    } while (0)
    int prev_dev = -1; /* the caller's current device is left as it was */
    if (hipGetDevice(&prev_dev) != hipSuccess) prev_dev = -1;
    CREATE_TRY(hipSetDevice(device));
    CREATE_TRY(hipGetDeviceProperties(&prop, device));
    c->knobs.n_cu = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
    if (const char *e = getenv("MCQ_SPLIT_MAX")) { /* tuning knob, see mcq_plan_geometry */
        int v = atoi(e);
        c->knobs.split_max = (uint32_t)(v < 0 ? 0 : (v > 4 ? 4 : v));
    }
    if (const char *e = getenv("MCQ_DIRECT_MAX_TASKS")) { /* tuning knob, see eval_host_philox */
        const int v = atoi(e);
        c->direct_max_tasks = (uint32_t)(v < 0 ? 0 : v > (int)MCQ_DIRECT_TASKS_LIMIT ? (int)MCQ_DIRECT_TASKS_LIMIT : v);
    }
    if (const char *e = getenv("MCQ_DIRECT_POLL")) c->direct_poll = atoi(e) != 0;
    if (const char *e = getenv("MCQ_DIRECT_SLEEP")) c->direct_sleep = atoi(e) != 0; /* see wait_ticket */
    if (const char *e = getenv("MCQ_EXT_SMALL")) c->ext_small = atoi(e) != 0; /* see mcq_eval_batch_ext */
    if (const char *e = getenv("MCQ_MT_BLOCKS")) c->mt_blocks = atoi(e) != 0;  /* see replay_batch_device */
    if (const char *e = getenv("MCQ_MT_BLOCKS_MARGIN")) c->mt_blocks_margin = atoi(e);
    if (const char *e = getenv("MCQ_MT_JUMP")) {
        c->mt_jump = atoi(e) != 0;
        c->mt_jump_always = atoi(e) == 2; /* (tests: every query of more than one segment, whatever the estimate says) */
    }
    if (const char *e = getenv("MCQ_DIRECT_UNIFORM_MIN")) { /* tuning knob, see eval_host_philox */
        const long v = atol(e);
        c->direct_uniform_min = (size_t)(v < 0 ? 0 : v);
    }
    if (const char *e = getenv("MCQ_PUBLISH_MAX_ROWS")) { /* tuning knob, see eval_host_philox */
        const long v = atol(e);
        c->publish_max_rows = (size_t)(v < 0 ? 0 : v);
    }
    if (const char *e = getenv("MCQ_LOAD_WAVES")) { /* tuning knob, see mcq_plan_geometry */
        const int v = atoi(e);
        c->knobs.load_waves = (uint32_t)(v < 1 ? 1 : (v > 16 ? 16 : v));
    }
    if (const char *e = getenv("MCQ_GRID_CAP")) { /* at most this many blocks in a sliced launch (tests), see mcq_plan_geometry */
        const long v = atol(e);
        if (v >= 1) c->knobs.grid_cap = (uint32_t)(v > 0x7fffffffL ? 0x7fffffffL : v);
    }
    if (const char *e = getenv("MCQ_EXACT_CU")) { /* the CU count the exact plans size their grids by, capped (tests), see exact_cu */
        const long v = atol(e);
        if (v >= 1) c->exact_cu = (uint32_t)(v > 0x7fffffffL ? 0x7fffffffL : v);
    }
    if (const char *e = getenv("MCQ_HERO_PRE_SLICE")) { /* table completions per launch of the preflop hero-range enumeration (tests) */
        const long long v = atoll(e);
        if (v >= 1) c->hero_pre_slice = mcq_exact_hero_pre_slice((uint64_t)v);
    }
    if (const char *e = getenv("MCQ_MATRIX_CHUNK")) { /* records per launch of mcq_exact_matrix (tests): the output does not depend on it */
        const long v = atol(e);
        if (v >= 1) c->matrix_chunk = (uint32_t)(v > (long)MCQ_MATRIX_MAX_BATCH ? (long)MCQ_MATRIX_MAX_BATCH : v);
    }
    if (const char *e = getenv("MCQ_REPLAY_DEVICE_BYTES")) { /* chunking of the parity mode's draw buffer (tests) */
        const long long v = atoll(e);
        if (v > 0) c->replay_device_bytes = (uint64_t)v;
    }
    CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (auto &sc : c->scratch) CREATE_TRY(hipEventCreateWithFlags(&sc.done, hipEventDisableTiming));
    c->scratch[0].stream = c->stream; /* slot 0: the context's own stream (host entries) */
    c->scratch[0].used = true;
    for (int i = 0; i < mcq_ctx::kRing; i++) {
        CREATE_TRY(hipEventCreate(&c->ev0[i]));
        CREATE_TRY(hipEventCreate(&c->ev1[i]));
    }
    CREATE_TRY(hipMalloc((void **)&c->d_luts, sizeof(McqTables)));
    CREATE_TRY(hipMemcpy(c->d_luts, tabs, sizeof(McqTables), hipMemcpyHostToDevice));
    for (int mode = 0; mode < 3; mode++) {
        int occ = 0;
        CREATE_TRY(mcq_eval_occupancy(mode, (int)MCQ_PLAN_BLOCK, &occ));
        c->knobs.occ[mode] = (uint32_t)(occ < 1 ? 1 : (occ > 8 ? 8 : occ));
    }
#undef CREATE_TRY
    delete tabs;
    if (prev_dev >= 0 && prev_dev != device) (void)hipSetDevice(prev_dev);
    return c;
}

int mcq_kernel_times(mcq_ctx *c, float *ms, int max_n) {
    if (!c || !ms || max_n < 0) return mcq_fail(MCQ_EINVAL, "mcq_kernel_times: bad argument");
    MCQ_ENTER(c, "mcq_kernel_times");
    return kernel_times_impl(c, ms, max_n);
}

}  // extern "C"

static int kernel_times_impl(mcq_ctx *c, float *ms, int max_n) {
    uint64_t have = c->n_timed < (uint64_t)mcq_ctx::kRing ? c->n_timed : (uint64_t)mcq_ctx::kRing;
    int n = (int)(have < (uint64_t)max_n ? have : (uint64_t)max_n);
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    if (n > 0) /* the one-launch path returns when the rows are out, a moment before the kernel has retired */
        HIP_TRY(hipEventSynchronize(c->ev1[(int)((c->n_timed - 1u) % mcq_ctx::kRing)]));
    for (int i = 0; i < n; i++) {
        int slot = (int)((c->n_timed - (uint64_t)n + (uint64_t)i) % mcq_ctx::kRing);
        HIP_TRY(hipEventElapsedTime(&ms[i], c->ev0[slot], c->ev1[slot]));
    }
    return n;
}

extern "C" {

int mcq_set_kernel_timing(mcq_ctx *c, int on) {
    if (!c) return mcq_fail(MCQ_EINVAL, "mcq_set_kernel_timing: null context");
    MCQ_ENTER(c, "mcq_set_kernel_timing");
    c->timing = on != 0;
    return MCQ_OK;
}

int mcq_set_dealing_law(mcq_ctx *c, int law) {
    if (!c || (law != MCQ_LAW_REFERENCE && law != MCQ_LAW_UNIFORM)) return mcq_fail(MCQ_EINVAL, "mcq_set_dealing_law: bad argument");
    MCQ_ENTER(c, "mcq_set_dealing_law");
    c->law = law;
    return MCQ_OK;
}

float mcq_last_kernel_ms(mcq_ctx *c) {
    float ms = 0.f;
    if (!c) return 0.f;
    McqBusyScope busy_(&c->busy);
    if (!busy_.ok) return 0.f; /* a call is running on the context: no time to report yet */
    if (c->last_ms > 0.f) return c->last_ms;
    if (!c->timing) return 0.f;
    return kernel_times_impl(c, &ms, 1) == 1 ? ms : 0.f;
}

int mcq_eval_batch_device(mcq_ctx *c, const void *d_queries, size_t n, uint64_t seed, uint64_t first_query_id,
                          void *d_results, void *hip_stream) {
    ABI_GUARD_BEGIN
    if (!c) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device: null context");
    if (n == 0) return MCQ_OK;
    if (!d_queries || !d_results) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device: null buffer");
    if (n > 0x7fffffffu) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device: n too large");
    MCQ_ENTER(c, "mcq_eval_batch_device");
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    hipStream_t s = (hipStream_t)hip_stream; /* NULL = the HIP null stream */
    /* the prefix buffer must already be large enough when the call is being captured into a graph */
    c->last_ms = 0.f;
    return mcq_run_slice(c, MCQ_MODE_PHILOX, (const mcq_query *)d_queries, (uint32_t)n, (mcq_result *)d_results, seed,
                     first_query_id, 0, nullptr, nullptr, s, true);
    ABI_GUARD_END("mcq_eval_batch_device")
}

/* The same with mcq_result_ways rows: the prep kernel clears 22 words per row, the evaluation kernel is the instantiation
 * that splits the ties (for up to 1024 small queries the finer cut the prep kernel picks). */
int mcq_eval_batch_device_ways(mcq_ctx *c, const void *d_queries, size_t n, uint64_t seed, uint64_t first_query_id,
                               void *d_results, void *hip_stream) {
    ABI_GUARD_BEGIN
    if (!c) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device_ways: null context");
    if (n == 0) return MCQ_OK;
    if (!d_queries || !d_results) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device_ways: null buffer");
    if (n > 0x7fffffffu) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device_ways: n too large");
    MCQ_ENTER(c, "mcq_eval_batch_device_ways");
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    c->last_ms = 0.f;
    return mcq_run_slice(c, MCQ_MODE_PHILOX, (const mcq_query *)d_queries, (uint32_t)n, (mcq_result *)d_results, seed,
                         first_query_id, 0, nullptr, nullptr, (hipStream_t)hip_stream, true, 0, 0, 1, nullptr, nullptr, nullptr,
                         kWaysWords);
    ABI_GUARD_END("mcq_eval_batch_device_ways")
}

/* Small queries resident in HBM -- the reference's call pattern (gym_env/env.py:22,261-262: 1000 runs per query) for a
 * caller whose states already live on the GPU: ONE kernel launch and nothing else (mcq_eval_direct_kernel in its device
 * mode): no prep kernel, no cost prefix, no atomics -- every query is owned by 2^lg waves of one block, lg chosen from
 * the query count alone, validation happens in the kernel. */
int mcq_eval_batch_device_small(mcq_ctx *c, const void *d_queries, size_t n, uint64_t seed, uint64_t first_query_id,
                                void *d_results, void *hip_stream) {
    ABI_GUARD_BEGIN
    if (!c) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device_small: null context");
    if (n == 0) return MCQ_OK;
    if (!d_queries || !d_results) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device_small: null buffer");
    if (n >= (1u << 24)) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device_small: n too large");
    MCQ_ENTER(c, "mcq_eval_batch_device_small");
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    hipStream_t s = (hipStream_t)hip_stream;
    const bool capturing = stream_capturing(s);
    /* the block counter of this stream (calls on different streams may overlap): a line of d_done_dev per scratch slot */
    if (!c->d_done_dev.p) {
        if (capturing)
            return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_device_small: issue one call on this context before capturing");
        HIP_TRY(c->d_done_dev.reserve(64 * mcq_ctx::kScratch));
        HIP_TRY(hipMemset(c->d_done_dev.p, 0, 64 * mcq_ctx::kScratch));
    }
    mcq_ctx::Scratch *sc = nullptr;
    int rc = scratch_for(c, s, 0, capturing, &sc);
    if (rc) return rc;
    uint32_t *d_done = reinterpret_cast<uint32_t *>(static_cast<char *>(c->d_done_dev.p) + 64 * (sc - c->scratch));
    const McqSmallCut cut = mcq_plan_small_cut(n, c->knobs.n_cu, c->knobs.split_max);
    const uint32_t mode = c->law == MCQ_LAW_UNIFORM ? MCQ_INTERNAL_MODE_UNIFORM : MCQ_MODE_PHILOX;
    const bool timed = c->timing && !capturing;
    const int slot = (int)(c->n_timed % mcq_ctx::kRing);
    c->last_ms = 0.f;
    HIP_TRY(mcq_launch_eval_direct((int)mode, d_queries, nullptr, cut.rounds, cut.lg ? 1u : 0u, (mcq_result *)d_results, seed, first_query_id,
                                   c->d_luts, cut.grid, d_done, d_done + 8 /* nobody polls: the stream orders the call */, 1u, s,
                                   timed ? c->ev0[slot] : nullptr, timed ? c->ev1[slot] : nullptr, nullptr, (uint32_t)n, cut.lg));
    if (timed) c->n_timed++;
    if (!capturing && sc != &c->scratch[0]) {
        HIP_TRY(hipEventRecord(sc->done, s));
        sc->done_recorded = true;
    }
    return MCQ_OK;
    ABI_GUARD_END("mcq_eval_batch_device_small")
}

/* The completion flag of the kernels that hand their rows over in pinned memory (mcq_eval_direct_kernel,
 * mcq_publish_kernel): a word the last block sets to the call's ticket, and the device counter that finds that block. */
static int flag_ready(mcq_ctx *c) {
    if (!c->h_flag.p) {
        HIP_TRY(c->h_flag.reserve(64));
        memset(c->h_flag.p, 0, 64);
        HIP_TRY(c->d_done.reserve(64));
        HIP_TRY(hipMemsetAsync(c->d_done.p, 0, 64, c->stream));
    }
    return MCQ_OK;
}
static uint32_t next_ticket(mcq_ctx *c) {
    if (++c->direct_ticket == 0u) c->direct_ticket = 1u; /* 0 is the flag's resting value */
    return c->direct_ticket;
}
/* Picking the rows up at the flag saves the end-of-kernel handshake of a stream synchronisation (24 us against 7.5 us
 * from launch to flag for an empty kernel, tools/launch_floor.hip).  Polling burns a core, so it is kept for SHORT
 * work: a call whose kernels are expected to run for est_us microseconds (scheduling cost x the measured time per cost
 * unit) first sleeps through most of that and only then polls; a kernel that has not answered a few milliseconds
 * after it was expected is left to hipStreamSynchronize, which reports what went wrong. */
static int wait_ticket(mcq_ctx *c, uint32_t ticket, bool *by_flag, double est_us) {
    const volatile uint32_t *flag = static_cast<const volatile uint32_t *>(c->h_flag.p);
    bool seen = false;
    if (c->direct_poll) {
        /* (half of the estimate: the constant behind est_us was measured on a whole MI355X under one dealing law; an
         * overshoot would add to the call what the flag was built to save.  MCQ_DIRECT_SLEEP=0: never sleep) */
        if (c->direct_sleep && est_us > 300.0) std::this_thread::sleep_for(std::chrono::microseconds((long long)(0.5 * est_us)));
        const auto t1 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0;; spin++) {
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket) { seen = true; break; }
            if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t1 > std::chrono::milliseconds(5)) break;
            __builtin_ia32_pause();
        }
    }
    if (!seen) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        /* late, or the flag never came: whatever the reason, the next launch starts from a clean block counter */
        if (c->direct_poll && __atomic_load_n(flag, __ATOMIC_ACQUIRE) != ticket)
            HIP_TRY(hipMemsetAsync(c->d_done.p, 0, 64, c->stream));
    }
    if (by_flag) *by_flag = seen;
    return MCQ_OK;
}
/* expected kernel time of work of scheduling cost `cost` (mcq_task_weight units, about 0.0066 ns each on a whole MI355X) */
static double cost_to_us(const mcq_ctx *c, uint64_t cost) { return (double)cost * 6.6e-6 * 256.0 / (double)(c->knobs.n_cu > 0 ? c->knobs.n_cu : 256); }

/* Production mode from host buffers.  The host has the queries in its hands, so it prices them itself: the cost
 * prefix travels with the queries in ONE copy, the result rows are zero already (every call leaves them so), and
 * the only kernel of the call is the evaluation kernel -- no prep launch on the path of the reference's own call
 * pattern, thousands of 1000-run queries (gym_env/env.py:22,261-262).  `runs` (and nothing else) of a row is the
 * host's to fill in. */
static int eval_host_philox(mcq_ctx *c, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id, uint32_t part,
                            uint32_t n_parts, void *out, const char *who, uint32_t rw) {
    const bool ways = rw == kWaysWords;
    if (!q || !out) return mcq_fail(MCQ_EINVAL, who, "null buffer");
    if (n > 0x7fffffffu) return mcq_fail(MCQ_EINVAL, who, "n too large");
    int rc = validate(q, n);
    if (rc) return rc;
    const size_t q_bytes = n * sizeof(mcq_query), p_bytes = (n + 3) * sizeof(uint64_t), r_bytes = n * rw * 8u;
    const size_t r_pad = (n + (n & 1u)) * rw * 8u; /* whole 16-byte words (mcq_publish_kernel) */
    /* behind the records: the cost prefix, then (one-launch path) the wave layout: at most n + 2 * 16 * n_cu waves, dealt
     * to the blocks in whole rounds */
    const size_t a_off = (q_bytes + p_bytes + 15u) & ~(size_t)15u, a_cap = n + 96u * (size_t)c->knobs.n_cu + 64u; /* waves */
    HIP_TRY(c->h_q.reserve(a_off + a_cap * (sizeof(mcq_query) + sizeof(uint32_t))));
    HIP_TRY(c->d_q.reserve(q_bytes + p_bytes));
    HIP_TRY(c->h_res.reserve(r_pad));
    if (r_pad > c->d_res.cap) c->res_clean = 0;
    HIP_TRY(c->d_res.reserve(r_pad));
    memcpy(c->h_q.p, q, q_bytes);
    uint64_t *prefix = reinterpret_cast<uint64_t *>(static_cast<char *>(c->h_q.p) + q_bytes);
    uint64_t total_tasks = 0, max_tasks = 0, cost = 0, unsplit = 0;
    for (size_t i = 0; i < n; i++) {
        const McqQueryWords w = mcq_query_words(q[i]);
        const McqPart pt = mcq_part(mcq_task_count(w), w.runs(), part, n_parts);
        const uint64_t t = pt.t_hi - pt.t_lo;
        prefix[i] = cost;
        cost += t * mcq_task_weight(w);
        total_tasks += t;
        unsplit += tasks_of(q[i]);
        if (t > max_tasks) max_tasks = t;
    }
    if (unsplit > 0xfffffff0ull) return mcq_fail(MCQ_EINVAL, who, "too many iterations in one call");
    if (n_parts == 1 && max_tasks <= c->direct_max_tasks && total_tasks > 0 && n < (1u << 24)) {
        /* Small queries -- the reference's call pattern: ONE launch (mcq_eval_direct_kernel).  The kernel reads the
         * records from this pinned buffer and stores finished rows into the pinned result buffer.  Layout of the work:
         * about 16 waves per CU in all, every query a power-of-two number of them in proportion to its cost (so all
         * waves carry about the same work), the waves of a query side by side in one block. */
        const uint32_t mode = c->law == MCQ_LAW_UNIFORM ? MCQ_INTERNAL_MODE_UNIFORM : MCQ_MODE_PHILOX;
        if (n >= c->direct_uniform_min && max_tasks <= 8u) {
            /* Many small queries: the kernel lays its own work out (its device mode, as mcq_eval_batch_device_small:
             * 2^lg waves per query from the query count alone) and reads the caller's records -- copied into this pinned
             * buffer, nothing else -- across PCIe: the host neither prices nor places a thousand queries (12 us), and a
             * uniform cut turned out no slower on the GPU than the cost-proportional one. */
            const McqSmallCut cut = mcq_plan_small_cut(n, c->knobs.n_cu, c->knobs.split_max);
            rc = flag_ready(c);
            if (rc) return rc;
            const uint32_t ticket = next_ticket(c);
            const int slot = (int)(c->n_timed % mcq_ctx::kRing);
            c->last_ms = 0.f;
            HIP_TRY(mcq_launch_eval_direct((int)mode, c->h_q.dev, nullptr, cut.rounds, cut.lg ? 1u : 0u, (mcq_result *)c->h_res.dev, seed,
                                           first_query_id, c->d_luts, cut.grid, (uint32_t *)c->d_done.p, (uint32_t *)c->h_flag.dev,
                                           ticket, c->stream, c->timing ? c->ev0[slot] : nullptr,
                                           c->timing ? c->ev1[slot] : nullptr, nullptr, (uint32_t)n, cut.lg, ways));
            if (c->timing) c->n_timed++;
            rc = wait_ticket(c, ticket, nullptr);
            if (rc) return rc;
            memcpy(out, c->h_res.p, r_bytes);
            return MCQ_OK;
        }
        std::vector<uint64_t> &qcost = c->direct_cost;
        qcost.resize(n);
        for (size_t i = 0; i < n; i++) qcost[i] = (i + 1 < n ? prefix[i + 1] : cost) - prefix[i];
        McqDirectLayout &lay = c->direct_layout;
        /* at most eight waves per query here: a sixteenth wave steps over fifteen iterations' words to run one
         * (tools/single_probe.py: one 1000-run query 1 us slower with sixteen, whatever the players and the table) */
        mcq_direct_layout(qcost.data(), n, c->knobs.n_cu, c->knobs.split_max < 3u ? c->knobs.split_max : 3u, lay);
        const uint32_t grid = lay.grid, rounds = lay.rounds;
        const size_t a_words = lay.slots;
        if (a_words > a_cap) return mcq_fail(MCQ_EDEVICE, who, "internal: wave layout larger than its bound");
        /* behind the caller's records and the prefix: one record copy per wave (its reserved bytes carry log2 of the
         * query's wave count and the wave's cut number), then one query index per wave */
        mcq_query *work_rec = reinterpret_cast<mcq_query *>(static_cast<char *>(c->h_q.p) + a_off);
        uint32_t *work_qi = reinterpret_cast<uint32_t *>(work_rec + a_words);
        /* a launch of few waves carries its work in the kernel arguments instead (no read across PCIe by the kernel) */
        const bool by_karg = a_words <= MCQ_DIRECT_KARG_SLOTS && rounds <= 8u;
        McqDirectKarg &karg = c->direct_karg;
        if (by_karg) {
            work_rec = reinterpret_cast<mcq_query *>(karg.rec);
            work_qi = karg.qi;
        }
        if (!mcq_direct_write_records(lay, q, n, work_rec, work_qi, by_karg ? (size_t)MCQ_DIRECT_KARG_SLOTS : a_cap))
            return mcq_fail(MCQ_EDEVICE, who, "internal: wave layout does not fit its slots");
        rc = flag_ready(c);
        if (rc) return rc;
        const uint32_t ticket = next_ticket(c);
        const int slot = (int)(c->n_timed % mcq_ctx::kRing);
        const bool timed = c->timing;
        c->last_ms = 0.f;
        static const bool trace = getenv("MCQ_TRACE") != nullptr; /* phase times of this path on stderr (tuning) */
        const auto t0 = std::chrono::steady_clock::now();
        const char *dev_rec = static_cast<const char *>(c->h_q.dev) + a_off;
        HIP_TRY(mcq_launch_eval_direct((int)mode, dev_rec,
                                       reinterpret_cast<const uint32_t *>(dev_rec + a_words * sizeof(mcq_query)), rounds,
                                       lay.merge ? 1u : 0u, (mcq_result *)c->h_res.dev, seed, first_query_id, c->d_luts, grid,
                                       (uint32_t *)c->d_done.p, (uint32_t *)c->h_flag.dev, ticket, c->stream,
                                       timed ? c->ev0[slot] : nullptr, timed ? c->ev1[slot] : nullptr,
                                       by_karg ? &karg : nullptr, 0, 0, ways));
        if (timed) c->n_timed++;
        const auto t1 = std::chrono::steady_clock::now();
        bool seen = false; /* the last block raises the flag once every row is out */
        rc = wait_ticket(c, ticket, &seen);
        if (rc) return rc;
        const auto t2 = std::chrono::steady_clock::now();
        memcpy(out, c->h_res.p, r_bytes);
        if (trace) {
            const auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
                return std::chrono::duration<double, std::micro>(b - a).count();
            };
            float kms = 0.f;
            if (timed) (void)kernel_times_impl(c, &kms, 1);
            fprintf(stderr, "mcq direct n=%zu waves=%llu grid=%u rounds=%u: launch %.1f us, wait %.1f us (%s), copy out %.1f us, "
                    "kernel %.1f us\n", n, (unsigned long long)lay.waves, grid, rounds, us(t0, t1), us(t1, t2),
                    seen ? "flag" : "stream sync", us(t2, std::chrono::steady_clock::now()), 1e3 * kms);
        }
        return MCQ_OK;
    }
    prefix[n] = cost;
    prefix[n + 1] = 0;
    prefix[n + 2] = 0;
    HIP_TRY(hipMemcpyAsync(c->d_q.p, c->h_q.p, q_bytes + p_bytes, hipMemcpyHostToDevice, c->stream));
    if (c->res_clean < r_pad) HIP_TRY(hipMemsetAsync(c->d_res.p, 0, r_pad, c->stream));
    c->res_clean = 0; /* dirty until this call has put its rows back to zero */
    c->last_ms = 0.f;
    if (total_tasks) {
        rc = mcq_run_slice(c, MCQ_MODE_PHILOX, (const mcq_query *)c->d_q.p, (uint32_t)n, (mcq_result *)c->d_res.p, seed,
                           first_query_id, total_tasks, nullptr, nullptr, c->stream, true, max_tasks, part, n_parts, nullptr,
                           reinterpret_cast<const uint64_t *>(static_cast<const char *>(c->d_q.p) + q_bytes), nullptr, rw);
        if (rc) return rc;
    }
    if (n <= c->publish_max_rows) {
        /* few rows: a small kernel behind the evaluation moves them into pinned memory, zeroes them in HBM for the next
         * call and raises the flag (no D2H copy, no stream synchronisation, no memset) */
        rc = flag_ready(c);
        if (rc) return rc;
        const uint32_t ticket = next_ticket(c);
        HIP_TRY(mcq_launch_publish((mcq_result *)c->d_res.p, (mcq_result *)c->h_res.dev, n + (n & 1u), (uint32_t *)c->d_done.p,
                                   (uint32_t *)c->h_flag.dev, ticket, c->stream, rw * 8u));
        rc = wait_ticket(c, ticket, nullptr, cost_to_us(c, cost));
        if (rc) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(c->h_res.p, c->d_res.p, r_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemsetAsync(c->d_res.p, 0, r_pad, c->stream)); /* not waited for: the next call finds its rows zero */
    }
    c->res_clean = r_pad;
    if (!total_tasks || !c->timing || kernel_times_impl(c, &c->last_ms, 1) != 1) c->last_ms = 0.f;
    memcpy(out, c->h_res.p, r_bytes);
    for (size_t i = 0; i < n; i++) row_at(out, i, rw)->runs = mcq_part(tasks_of(q[i]), q[i].runs, part, n_parts).runs;
    return MCQ_OK;
}

static int eval_batch_impl(mcq_ctx *c, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id, int mode,
                           uint32_t part, uint32_t n_parts, void *out, const char *who, uint32_t rw = kPlainWords) {
    if (mode != MCQ_MODE_PHILOX && mode != MCQ_MODE_REPLAY_MT19937) return mcq_fail(MCQ_EINVAL, who, "bad mode");
    if (n_parts == 0 || part >= n_parts) return mcq_fail(MCQ_EINVAL, who, "part must be < n_parts");
    if (n_parts > 1 && mode != MCQ_MODE_PHILOX)
        return mcq_fail(MCQ_EINVAL, who, "only MCQ_MODE_PHILOX can split the iterations of a query");
    if (n == 0) return MCQ_OK;
    if (!c) return mcq_fail(MCQ_EINVAL, who, "null context");
    MCQ_ENTER(c, who);
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    if (mode == MCQ_MODE_PHILOX) return eval_host_philox(c, q, n, seed, first_query_id, part, n_parts, out, who, rw);
    int rc = stage_queries(c, q, n, out, who, rw);
    if (rc) return rc;
    return replay_batch(c, q, n, seed, first_query_id, nullptr, static_cast<mcq_result *>(out), rw);
}

int mcq_eval_batch(mcq_ctx *c, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id, int mode,
                   mcq_result *out) {
    ABI_GUARD_BEGIN
    return eval_batch_impl(c, q, n, seed, first_query_id, mode, 0, 1, out, "mcq_eval_batch");
    ABI_GUARD_END("mcq_eval_batch")
}

int mcq_eval_batch_ways(mcq_ctx *c, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id, int mode,
                        mcq_result_ways *out) {
    ABI_GUARD_BEGIN
    return eval_batch_impl(c, q, n, seed, first_query_id, mode, 0, 1, out, "mcq_eval_batch_ways", kWaysWords);
    ABI_GUARD_END("mcq_eval_batch_ways")
}

int mcq_eval_batch_part(mcq_ctx *c, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id,
                        uint32_t part, uint32_t n_parts, mcq_result *out) {
    ABI_GUARD_BEGIN
    return eval_batch_impl(c, q, n, seed, first_query_id, MCQ_MODE_PHILOX, part, n_parts, out, "mcq_eval_batch_part");
    ABI_GUARD_END("mcq_eval_batch_part")
}

int mcq_eval_one(mcq_ctx *c, const mcq_query *q, uint64_t seed, int mode, mcq_result *out) {
    return mcq_eval_batch(c, q, 1, seed, 0, mode, out);
}

}  // extern "C"

/* mcq_eval_batch_ext, mcq_eval_batch_ext_ways and mcq_eval_batch_ext_seats: rw = 64-bit words of a result row (out ->
 * rows of that length).  The per-seat rows: production mode only, always the general path. */
static int eval_batch_ext_impl(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, uint64_t seed,
                               uint64_t first_query_id, int mode, void *out, uint32_t rw) {
    const bool ways = rw == kWaysWords, seats = rw == kSeatsWords;
    const size_t row_bytes = (size_t)rw * 8u;
    if (mode != MCQ_MODE_PHILOX && mode != MCQ_MODE_REPLAY_MT19937) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: bad mode");
    if (seats && mode != MCQ_MODE_PHILOX)
        return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext_seats: MCQ_MODE_PHILOX only (the per-seat rows have no parity form)");
    if (n == 0) return MCQ_OK;
    if (!c) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: null context");
    if (!q || !ext || !out) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: null buffer");
    if (n > 0x7fffffffu) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: n too large");
    /* the extended kernels deal the reference's law only: refuse rather than deal it under the uniform law's name */
    if (mode == MCQ_MODE_PHILOX && c->law == MCQ_LAW_UNIFORM)
        return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: the uniform dealing law is not available for extended queries "
                                    "(exact enumeration has it: mcq_exact_batch_ext)");
    uint64_t total_tasks = 0;
    uint32_t lists_stride = 1; /* candidate lists per query of the production mode: the batch's maximum */
    uint32_t most_tasks = 0;
    for (size_t i = 0; i < n; i++) {
        const McqExtRec er = {reinterpret_cast<const uint32_t *>(&ext[i])};
        const McqQueryWords qw = mcq_query_words(q[i]);
        if (!mcq_query_ext_valid(qw, er)) {
            char buf[220];
            snprintf(buf, sizeof buf, "extended query %zu invalid (distinct card ids < 52 among hole/table/ghost/known hands, "
                     "at most 9 further known hands, n_players >= known hands, used ranges not empty)", i);
            return mcq_fail(MCQ_EINVAL, buf);
        }
        const uint32_t nl = mcq_ext_n_lists(qw, er);
        if (nl > lists_stride) lists_stride = nl;
        const uint32_t t = mcq_ext_task_count(qw, mode == MCQ_MODE_PHILOX ? mcq_ext_stream_iters(qw, er) : MCQ_STREAM_ITERS);
        total_tasks += t;
        if (t > most_tasks) most_tasks = t;
    }
    if (total_tasks > 0xfffffff0ull) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: too many iterations in one call");
    MCQ_ENTER(c, "mcq_eval_batch_ext");
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    HIP_TRY(c->h_res.reserve(n * row_bytes));
    if (!seats && mode == MCQ_MODE_PHILOX && c->ext_small && mcq_ext_small_fits(n, lists_stride, most_tasks) &&
        !stream_capturing(c->stream)) {
        /* what a decision of the reference's agents asks for -- one ranged query of a thousand iterations -- in ONE
         * launch: the records in the kernel arguments, a block per query (lists laid out in its LDS), the rows into
         * pinned memory, the flag: 140 -> ~25 us per call */
        static_assert(sizeof(mcq_query_ext) == sizeof(((McqExtSmallKarg *)0)->ext[0]), "extension record in the kernel arguments");
        McqExtSmallKarg karg;
        uint32_t tasks[MCQ_EXT_SMALL_Q];
        for (size_t i = 0; i < n; i++) {
            memcpy(karg.q[i], &q[i], sizeof(mcq_query));
            memcpy(karg.ext[i], &ext[i], sizeof(mcq_query_ext));
            const McqExtRec er = {reinterpret_cast<const uint32_t *>(&ext[i])};
            const McqQueryWords qw = mcq_query_words(q[i]);
            tasks[i] = mcq_ext_task_count(qw, mcq_ext_stream_iters(qw, er));
        }
        const McqExtSmallPlan plan = mcq_ext_small_plan(tasks, (uint32_t)n, karg.blk);
        HIP_TRY(c->h_res.reserve(MCQ_EXT_SMALL_BLOCKS * row_bytes));
        int rc = flag_ready(c);
        if (rc) return rc;
        const uint32_t ticket = next_ticket(c);
        const int slot = (int)(c->n_timed % mcq_ctx::kRing);
        const bool timed = c->timing;
        c->last_ms = 0.f;
        HIP_TRY(mcq_launch_eval_ext_small(&karg, plan.n_blocks, (mcq_result *)c->h_res.dev, seed, first_query_id, c->d_luts,
                                          (uint32_t *)c->d_done.p, (uint32_t *)c->h_flag.dev, ticket, c->stream,
                                          timed ? c->ev0[slot] : nullptr, timed ? c->ev1[slot] : nullptr, ways));
        if (timed) c->n_timed++;
        rc = wait_ticket(c, ticket, nullptr);
        if (rc) return rc;
        if (timed && kernel_times_impl(c, &c->last_ms, 1) != 1) c->last_ms = 0.f;
        const uint64_t *hr = (const uint64_t *)c->h_res.p; /* one row (13 or 22 words) per block */
        static_assert(sizeof(mcq_result) == 13 * sizeof(uint64_t), "result row");
        for (size_t i = 0; i < n; i++) /* all rows first: an undealable range leaves `out` untouched */
            for (uint32_t b = plan.first_block[i]; b < plan.first_block[i + 1]; b++)
                if (hr[(size_t)rw * b] != q[i].runs)
                    return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: a range cannot be dealt from the remaining cards");
        for (size_t i = 0; i < n; i++) {
            uint64_t row[kWaysWords] = {q[i].runs};
            for (uint32_t b = plan.first_block[i]; b < plan.first_block[i + 1]; b++)
                for (uint32_t k = 1; k < rw; k++) row[k] += hr[(size_t)rw * b + k];
            memcpy(static_cast<uint8_t *>(out) + i * row_bytes, row, row_bytes);
        }
        return MCQ_OK;
    }
    HIP_TRY(c->h_q.reserve(n * (sizeof(mcq_query) + sizeof(mcq_query_ext))));
    HIP_TRY(c->d_q.reserve(n * sizeof(mcq_query)));
    HIP_TRY(c->d_ext.reserve(n * sizeof(mcq_query_ext)));
    HIP_TRY(c->d_res.reserve(n * row_bytes));
    c->res_clean = 0;
    HIP_TRY(c->scratch[0].prefix.reserve((n + 3) * sizeof(uint64_t)));
    uint8_t *hq = (uint8_t *)c->h_q.p;
    memcpy(hq, q, n * sizeof(mcq_query));
    memcpy(hq + n * sizeof(mcq_query), ext, n * sizeof(mcq_query_ext));
    HIP_TRY(hipMemcpyAsync(c->d_q.p, hq, n * sizeof(mcq_query), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_ext.p, hq + n * sizeof(mcq_query), n * sizeof(mcq_query_ext), hipMemcpyHostToDevice,
                           c->stream));
    c->last_ms = 0.f;
    const McqGeometry geo = mcq_plan_geometry(c->knobs, mode, total_tasks);
    if (mode == MCQ_MODE_REPLAY_MT19937) {
        /* the draw buffer the stream walk fills and the evaluation kernel reads (one chunk: the extended path is a
         * feature path, not a bulk path); the walk itself runs on the device: mcq_mt_parse_ext_kernel, one wave per query */
        HIP_TRY(c->h_off.reserve(n * sizeof(uint64_t)));
        uint64_t *off = (uint64_t *)c->h_off.p, bytes = 0;
        for (size_t i = 0; i < n; i++) {
            off[i] = bytes;
            bytes += (((uint64_t)q[i].runs + 63u) & ~63ull) * mcq_ext_draws_per_iteration(q[i], ext[i]);
        }
        if (bytes > (1ull << 32)) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: replay batch too large (split it)");
        HIP_TRY(c->d_draws.reserve(bytes + 64));
        HIP_TRY(c->d_off.reserve(n * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(c->d_off.p, off, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(mcq_launch_prep_ext((const mcq_query *)c->d_q.p, (const mcq_query_ext *)c->d_ext.p, (uint32_t)n, mode,
                                (mcq_result *)c->d_res.p, (uint64_t *)c->scratch[0].prefix.p, c->stream, rw));
    const int slot = (int)(c->n_timed % mcq_ctx::kRing);
    hipEvent_t t0 = c->timing ? c->ev0[slot] : nullptr; /* parity mode: the timed region starts in front of the stream walk */
    if (mode == MCQ_MODE_REPLAY_MT19937) {
        if (t0) HIP_TRY(hipEventRecord(t0, c->stream));
        t0 = nullptr;
        HIP_TRY(mcq_launch_mt_parse_ext((const mcq_query *)c->d_q.p, (const mcq_query_ext *)c->d_ext.p, (uint32_t)n,
                                        (uint32_t)(seed + first_query_id), (uint8_t *)c->d_draws.p, (const uint64_t *)c->d_off.p,
                                        (mcq_result *)c->d_res.p,
                                        reinterpret_cast<uint32_t *>((uint64_t *)c->scratch[0].prefix.p + n + 2), c->knobs.n_cu,
                                        c->stream, rw));
    }
    if (mode == MCQ_MODE_PHILOX) { /* the candidate lists of the ranges, once per query */
        HIP_TRY(c->d_lists.reserve(n * (size_t)lists_stride * MCQ_EXT_LIST_STRIDE * sizeof(uint16_t)));
        HIP_TRY(c->d_cnts.reserve(n * (size_t)lists_stride * sizeof(uint32_t)));
        HIP_TRY(mcq_launch_ext_lists((const mcq_query *)c->d_q.p, (const mcq_query_ext *)c->d_ext.p, (uint32_t)n, lists_stride,
                                     (uint16_t *)c->d_lists.p, (uint32_t *)c->d_cnts.p, c->stream));
    }
    HIP_TRY(mcq_launch_eval_ext(mode, (const mcq_query *)c->d_q.p, (const mcq_query_ext *)c->d_ext.p, (uint32_t)n,
                                (const uint64_t *)c->scratch[0].prefix.p, (mcq_result *)c->d_res.p, seed, first_query_id, c->d_luts,
                                (const uint8_t *)c->d_draws.p, (const uint64_t *)c->d_off.p, (const uint16_t *)c->d_lists.p,
                                (const uint32_t *)c->d_cnts.p, lists_stride, geo.grid, geo.block, c->stream,
                                t0, c->timing ? c->ev1[slot] : nullptr, ways, seats));
    if (c->timing) c->n_timed++;
    HIP_TRY(hipMemcpyAsync(c->h_res.p, c->d_res.p, n * row_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!c->timing || kernel_times_impl(c, &c->last_ms, 1) != 1) c->last_ms = 0.f;
    const uint64_t *hr = (const uint64_t *)c->h_res.p;
    for (size_t i = 0; i < n; i++) /* word 0 runs, word 1 passes (parity mode: the stream walk marks such a query) */
        if (hr[(size_t)rw * i] != q[i].runs || hr[(size_t)rw * i + 1u] == ~0ull)
            return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_ext: a range cannot be dealt from the remaining cards");
    memcpy(out, hr, n * row_bytes);
    return MCQ_OK;
}

extern "C" {

int mcq_eval_batch_ext(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, uint64_t seed,
                       uint64_t first_query_id, int mode, mcq_result *out) {
    ABI_GUARD_BEGIN
    return eval_batch_ext_impl(c, q, ext, n, seed, first_query_id, mode, out, kPlainWords);
    ABI_GUARD_END("mcq_eval_batch_ext")
}

int mcq_eval_batch_ext_ways(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, uint64_t seed,
                            uint64_t first_query_id, int mode, mcq_result_ways *out) {
    ABI_GUARD_BEGIN
    return eval_batch_ext_impl(c, q, ext, n, seed, first_query_id, mode, out, kWaysWords);
    ABI_GUARD_END("mcq_eval_batch_ext_ways")
}

int mcq_eval_batch_ext_seats(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, uint64_t seed,
                             uint64_t first_query_id, int mode, mcq_result_seats *out) {
    ABI_GUARD_BEGIN
    return eval_batch_ext_impl(c, q, ext, n, seed, first_query_id, mode, out, kSeatsWords);
    ABI_GUARD_END("mcq_eval_batch_ext_seats")
}

}  // extern "C"

/* A weighted range per seat (mcq_ranges.hpp): mcq_eval_batch_ranges and, per_hand, mcq_eval_batch_ranges_hands with the
 * watched seat's tally per hand (mcq_hands.hpp).  Everything that can be refused is refused here, before a launch; what
 * is left for the device is the record whose seats block each other. */
static int eval_batch_ranges_impl(const char *who, mcq_ctx *c, const mcq_query *q, const uint32_t *seat_table,
                                  const uint16_t *tables, size_t n_tables, size_t n, uint64_t seed, uint64_t first_query_id,
                                  mcq_result_seats *out, bool per_hand, uint32_t seat, mcq_hand_row *hands) {
    if (n == 0) return MCQ_OK;
    if (!c) return mcq_fail(MCQ_EINVAL, who, "null context");
    if (!q || !seat_table || !tables || !out || (per_hand && !hands)) return mcq_fail(MCQ_EINVAL, who, "null buffer");
    if (n > 0x7fffffffu) return mcq_fail(MCQ_EINVAL, who, "n too large");
    if (per_hand && n > MCQ_RANGES_HANDS_MAX_BATCH) return mcq_fail(MCQ_EINVAL, who, "n above MCQ_RANGES_HANDS_MAX_BATCH (split the batch)");
    if (n_tables == 0 || n_tables > 0x7fffffffu / MCQ_RG_CUM_STRIDE)
        return mcq_fail(MCQ_EINVAL, who, "n_tables must be 1 .. 2^31 / 1328");
    std::vector<uint32_t> with_card(n_tables * MCQ_RG_WITH_CARD_STRIDE);
    for (size_t t = 0; t < n_tables; t++) mcq_ranges_with_card(tables + t * MCQ_HAND_ROWS, with_card.data() + t * MCQ_RG_WITH_CARD_STRIDE);
    uint64_t total_tasks = 0;
    char buf[200];
    std::vector<uint32_t> price(n); /* estimated whole trials per iteration, for the cost axis only */
    for (size_t i = 0; i < n; i++) {
        const McqQueryWords qw = mcq_query_words(q[i]);
        if (!mcq_ranges_query_valid(qw)) {
            snprintf(buf, sizeof buf, "record %zu invalid (0, 3, 4 or 5 distinct table cards < 52, "
                     "n_players 2..10, reserved 0, runs >= 1)", i);
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
        const McqRangesPrice pr = mcq_ranges_price(tables, n_tables, with_card.data(), qw, seat_table + i * 10u);
        if (pr.refused == MCQ_RG_REFUSED_TABLE) {
            snprintf(buf, sizeof buf, "record %zu, seat %u names table %u of %zu", i, pr.seat, pr.table, n_tables);
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
        if (pr.refused) {
            snprintf(buf, sizeof buf, "record %zu, seat %u: table %u has no hand of positive weight "
                     "clear of the table cards", i, pr.seat, pr.table);
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
        if (per_hand && seat >= qw.n_players()) {
            snprintf(buf, sizeof buf, "record %zu has %u seats: no seat %u to watch", i, qw.n_players(), seat);
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
        price[i] = pr.price;
        total_tasks += mcq_ranges_task_count(qw);
    }
    if (total_tasks > 0xfffffff0ull) return mcq_fail(MCQ_EINVAL, who, "too many iterations in one call");
    MCQ_ENTER(c, who);
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    const size_t row_bytes = sizeof(mcq_result_seats), hand_bytes = n * MCQ_HAND_ROWS * sizeof(mcq_hand_row);
    HIP_TRY(c->h_res.reserve(n * row_bytes));
    HIP_TRY(c->d_q.reserve(n * sizeof(mcq_query)));
    HIP_TRY(c->d_res.reserve(n * row_bytes));
    c->res_clean = 0;
    HIP_TRY(c->scratch[0].prefix.reserve((n + 3) * sizeof(uint64_t)));
    /* (buffers of the extended path, free while this call runs: the raw tables, the prepared tables, the seats' table numbers) */
    HIP_TRY(c->d_lists.reserve(n_tables * MCQ_HAND_ROWS * sizeof(uint16_t)));
    HIP_TRY(c->d_draws.reserve(n_tables * MCQ_RG_CUM_STRIDE * sizeof(uint32_t)));
    HIP_TRY(c->d_cnts.reserve(n * 11u * sizeof(uint32_t))); /* ... and behind them the records' prices */
    if (per_hand) HIP_TRY(c->d_ext.reserve(hand_bytes)); /* ... the rows per hand: 42 KB per record */
    HIP_TRY(hipMemcpyAsync(c->d_q.p, q, n * sizeof(mcq_query), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_lists.p, tables, n_tables * MCQ_HAND_ROWS * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_cnts.p, seat_table, n * 10u * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((uint32_t *)c->d_cnts.p + n * 10u, price.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    c->last_ms = 0.f;
    const McqGeometry geo = mcq_plan_geometry(c->knobs, MCQ_MODE_PHILOX, total_tasks);
    const int slot = (int)(c->n_timed % mcq_ctx::kRing);
    if (per_hand)
        HIP_TRY(mcq_launch_eval_ranges_hands((const mcq_query *)c->d_q.p, (const uint32_t *)c->d_cnts.p,
                                             (const uint32_t *)c->d_cnts.p + n * 10u, (const uint16_t *)c->d_lists.p,
                                             (uint32_t)n_tables, (uint32_t *)c->d_draws.p, (uint32_t)n,
                                             (uint64_t *)c->scratch[0].prefix.p, (mcq_result *)c->d_res.p, (mcq_hand_row *)c->d_ext.p,
                                             seat, seed, first_query_id, c->d_luts, geo.grid, geo.block, c->stream,
                                             c->timing ? c->ev0[slot] : nullptr, c->timing ? c->ev1[slot] : nullptr));
    else
        HIP_TRY(mcq_launch_eval_ranges((const mcq_query *)c->d_q.p, (const uint32_t *)c->d_cnts.p,
                                       (const uint32_t *)c->d_cnts.p + n * 10u, (const uint16_t *)c->d_lists.p,
                                       (uint32_t)n_tables, (uint32_t *)c->d_draws.p, (uint32_t)n, (uint64_t *)c->scratch[0].prefix.p,
                                       (mcq_result *)c->d_res.p, seed, first_query_id, c->d_luts, geo.grid, geo.block, c->stream,
                                       c->timing ? c->ev0[slot] : nullptr, c->timing ? c->ev1[slot] : nullptr));
    if (c->timing) c->n_timed++;
    HIP_TRY(hipMemcpyAsync(c->h_res.p, c->d_res.p, n * row_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!c->timing || kernel_times_impl(c, &c->last_ms, 1) != 1) c->last_ms = 0.f;
    const uint64_t *hr = (const uint64_t *)c->h_res.p;
    for (size_t i = 0; i < n; i++)
        if (hr[(size_t)kSeatsWords * i] != q[i].runs)
            return mcq_fail(MCQ_EINVAL, who, "the seats' ranges block each other: an iteration found no "
                                             "trial in which their hands are disjoint");
    if (per_hand) { /* (behind the check: a refused call leaves both outputs untouched) */
        HIP_TRY(hipMemcpyAsync(hands, c->d_ext.p, hand_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    memcpy(out, hr, n * row_bytes);
    return MCQ_OK;
}

extern "C" {

int mcq_eval_batch_ranges(mcq_ctx *c, const mcq_query *q, const uint32_t *seat_table, const uint16_t *tables, size_t n_tables,
                          size_t n, uint64_t seed, uint64_t first_query_id, mcq_result_seats *out) {
    ABI_GUARD_BEGIN
    return eval_batch_ranges_impl("mcq_eval_batch_ranges", c, q, seat_table, tables, n_tables, n, seed, first_query_id, out,
                                  false, 0u, nullptr);
    ABI_GUARD_END("mcq_eval_batch_ranges")
}

int mcq_eval_batch_ranges_hands(mcq_ctx *c, const mcq_query *q, const uint32_t *seat_table, const uint16_t *tables,
                                size_t n_tables, size_t n, uint64_t seed, uint64_t first_query_id, uint32_t seat,
                                mcq_result_seats *out, mcq_hand_row *hands) {
    ABI_GUARD_BEGIN
    return eval_batch_ranges_impl("mcq_eval_batch_ranges_hands", c, q, seat_table, tables, n_tables, n, seed, first_query_id,
                                  out, true, seat, hands);
    ABI_GUARD_END("mcq_eval_batch_ranges_hands")
}

int mcq_eval_batch_numpy_stream(mcq_ctx *c, const mcq_query *q, size_t n, uint32_t *mt_key, uint32_t *mt_pos,
                                mcq_result *out) {
    ABI_GUARD_BEGIN
    if (n == 0) return MCQ_OK;
    if (!mt_key || !mt_pos || *mt_pos > 624) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_numpy_stream: bad MT19937 state");
    if (!c) return mcq_fail(MCQ_EINVAL, "mcq_eval_batch_numpy_stream: null context");
    MCQ_ENTER(c, "mcq_eval_batch_numpy_stream");
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    int rc = stage_queries(c, q, n, out, "mcq_eval_batch_numpy_stream");
    if (rc) return rc;
    McqMt19937 g;
    memcpy(g.mt, mt_key, sizeof g.mt);
    g.pos = *mt_pos;
    rc = replay_batch(c, q, n, 0, 0, &g, out);
    if (rc) return rc;
    memcpy(mt_key, g.mt, sizeof g.mt);
    *mt_pos = g.pos;
    return MCQ_OK;
    ABI_GUARD_END("mcq_eval_batch_numpy_stream")
}

int mcq_showdown(mcq_ctx *c, const uint8_t *hands, size_t n_tables, int n_players, uint8_t *winner,
                 uint8_t *winner_type, uint32_t *keys) {
    ABI_GUARD_BEGIN
    if (!c) return mcq_fail(MCQ_EINVAL, "mcq_showdown: null context");
    if (n_tables == 0) return MCQ_OK;
    if (!hands || !winner || !winner_type) return mcq_fail(MCQ_EINVAL, "mcq_showdown: null buffer");
    if (n_players < 1 || n_players > 10) return mcq_fail(MCQ_EINVAL, "mcq_showdown: n_players must be in [1,10]");
    if (n_tables > 0x7fffffffu / 70u) return mcq_fail(MCQ_EINVAL, "mcq_showdown: n_tables too large");
    /* The host only moves bytes: the hands go through pinned memory in pieces, each piece's kernel launched as soon as
     * the piece is there (the kernel reads it in place across PCIe with 16-byte loads while the host copies the next
     * piece), validation happens on the device, winners / types / keys come back in pinned memory and the last kernel
     * raises the completion flag -- no blocking copies, no stream synchronisation. */
    const size_t per_table = 7u * (size_t)n_players, nh = n_tables * (size_t)n_players;
    const size_t pad_tables = (n_tables + 255u) & ~(size_t)255u;
    const size_t in_bytes = pad_tables * per_table, key_bytes = keys ? pad_tables * n_players * sizeof(uint32_t) : 0;
    MCQ_ENTER(c, "mcq_showdown");
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    HIP_TRY(c->h_misc.reserve(in_bytes + 2 * pad_tables + key_bytes + 64));
    int rc = flag_ready(c);
    if (rc) return rc;
    uint8_t *hp = (uint8_t *)c->h_misc.p, *dp = (uint8_t *)c->h_misc.dev;
    const size_t off_w = in_bytes, off_t = off_w + pad_tables, off_k = off_t + pad_tables; /* all multiples of 16 */
    volatile uint32_t *bad = static_cast<volatile uint32_t *>(c->h_flag.p) + 1;
    *bad = 0;
    size_t piece = (256u << 10) / per_table & ~(size_t)255u; /* tables per piece: about 256 KB, whole tiles */
    if (piece < 256u) piece = 256u;
    const uint32_t ticket = next_ticket(c);
    for (size_t a = 0; a < n_tables; a += piece) {
        const size_t b = a + piece < n_tables ? a + piece : n_tables;
        memcpy(hp + a * per_table, hands + a * per_table, (b - a) * per_table);
        HIP_TRY(mcq_launch_showdown(dp + a * per_table, (uint32_t)(b - a), (uint32_t)n_players, c->d_luts, dp + off_w + a,
                                    dp + off_t + a, keys ? reinterpret_cast<uint32_t *>(dp + off_k) + a * n_players : nullptr,
                                    static_cast<uint32_t *>(c->h_flag.dev) + 1, (uint32_t *)c->d_done.p,
                                    (uint32_t *)c->h_flag.dev, b == n_tables ? ticket : 0u, c->knobs.n_cu, c->stream));
    }
    rc = wait_ticket(c, ticket, nullptr);
    if (rc) return rc;
    if (__atomic_load_n(bad, __ATOMIC_ACQUIRE) != 0u)
        return mcq_fail(MCQ_EINVAL, "mcq_showdown: a hand needs 7 distinct card ids < 52");
    memcpy(winner, hp + off_w, n_tables);
    memcpy(winner_type, hp + off_t, n_tables);
    if (keys) memcpy(keys, hp + off_k, nh * sizeof(uint32_t));
    return MCQ_OK;
    ABI_GUARD_END("mcq_showdown")
}

/* the CU count mcq_exact_plan and mcq_exact_ext_plan size a grid by: the device's, or MCQ_EXACT_CU where that is smaller */
static uint32_t exact_cu(const mcq_ctx *c) {
    return c->exact_cu && c->exact_cu < c->knobs.n_cu ? c->exact_cu : c->knobs.n_cu;
}

int mcq_exact_batch(mcq_ctx *c, const mcq_query *q, size_t n, int law, mcq_result *out) {
    ABI_GUARD_BEGIN
    if (!c) return mcq_fail(MCQ_EINVAL, "mcq_exact_batch: null context");
    if (n == 0) return MCQ_OK;
    if (!q || !out) return mcq_fail(MCQ_EINVAL, "mcq_exact_batch: null buffer");
    if (law != MCQ_LAW_REFERENCE && law != MCQ_LAW_UNIFORM) return mcq_fail(MCQ_EINVAL, "mcq_exact_batch: bad law");
    if (n > 0x7fffffffu) return mcq_fail(MCQ_EINVAL, "mcq_exact_batch: n too large");
    int rc = validate(q, n);
    if (rc) return rc;
    for (size_t i = 0; i < n; i++)
        if (q[i].n_players > 3)
            return mcq_fail(MCQ_EINVAL, "mcq_exact_batch: exact enumeration covers 1 to 3 players");
    MCQ_ENTER(c, "mcq_exact_batch");
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    HIP_TRY(c->d_res.reserve(n * sizeof(mcq_result)));
    c->res_clean = 0;
    HIP_TRY(c->h_res.reserve(n * sizeof(mcq_result)));
    HIP_TRY(hipMemsetAsync(c->d_res.p, 0, n * sizeof(mcq_result), c->stream));
    /* one launch per kind (two opponents / fewer) and 65 535 queries: the jobs travel in pinned memory */
    HIP_TRY(c->h_misc.reserve(n * sizeof(McqExactJob)));
    McqExactJob *jobs = static_cast<McqExactJob *>(c->h_misc.p);
    const McqExactJob *d_jobs = static_cast<const McqExactJob *>(c->h_misc.dev);
    size_t n_two = 0;
    for (size_t i = 0; i < n; i++) /* the two-opponent queries first, the others behind them */
        if (q[i].n_players == 3) mcq_exact_plan(&q[i], (uint32_t)i, exact_cu(c), &jobs[n_two++]);
    size_t at = n_two;
    for (size_t i = 0; i < n; i++)
        if (q[i].n_players != 3) mcq_exact_plan(&q[i], (uint32_t)i, exact_cu(c), &jobs[at++]);
    for (size_t a = 0; a < n;) {
        const bool two = a < n_two;
        const size_t end = two ? n_two : n, b = a + 65535u < end ? a + 65535u : end;
        uint32_t max_grid = 0;
        for (size_t i = a; i < b; i++) max_grid = jobs[i].grid > max_grid ? jobs[i].grid : max_grid;
        HIP_TRY(mcq_launch_exact(d_jobs + a, (uint32_t)(b - a), max_grid, two, law, (mcq_result *)c->d_res.p, c->d_luts, c->stream));
        a = b;
    }
    HIP_TRY(hipMemcpyAsync(c->h_res.p, c->d_res.p, n * sizeof(mcq_result), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(out, c->h_res.p, n * sizeof(mcq_result));
    return MCQ_OK;
    ABI_GUARD_END("mcq_exact_batch")
}

}  // extern "C"

/* Validation of a batch of extended records for exact enumeration, shared by exact_batch_ext_impl and
 * mcq_exact_batch_ext_runouts; nothing is launched for a batch with one record that cannot be enumerated.  build(words,
 * record, query) is the entry's query builder: it returns MCQ_XX_OK or why not -- below 5 one of the shared reasons, from 5
 * on more[why - 5].  Then the dealability check, then refuse(i, query) with what only the entry refuses (its text, or
 * nullptr).  -> xq[n] and the decks' card ids rid[64 n]. */
template <class Build, class Refuse>
static int exact_ext_validate(const mcq_query *q, const mcq_query_ext *ext, size_t n, const char *who, Build build,
                              const char *const *more, Refuse refuse, std::vector<McqExactExtQuery> &xq, std::vector<uint8_t> &rid) {
    static const char *const reason[] = {
        "", "invalid extended query (as mcq_eval_batch_ext: distinct card ids < 52, at most 9 known hands, used ranges not empty)",
        "a hero range is not enumerated (rotate a known hand into the hero's seat)",
        "a known hand given as a range is not enumerated", "at most two random opponents"};
    xq.resize(n);
    rid.resize(n * 64u);
    for (size_t i = 0; i < n; i++) {
        const McqExtRec er = {reinterpret_cast<const uint32_t *>(&ext[i])};
        const int why = build(mcq_query_words(q[i]), er, xq[i]);
        const char *text = why == MCQ_XX_OK ? nullptr : why < 5 ? reason[why] : more[why - 5];
        if (!text) {
            mcq_exact_ext_r_ids(xq[i], &rid[64u * i]);
            text = !mcq_exact_ext_dealable(xq[i], &rid[64u * i]) ? "the opponents' range cannot be dealt from the remaining cards"
                                                                 : refuse(i, xq[i]);
        }
        if (text) {
            char buf[200];
            snprintf(buf, sizeof buf, "query %zu: %s", i, text);
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
    }
    return MCQ_OK;
}

/* ... and their staging: jobs and extension records travel in pinned memory, the jobs grouped by kind = random opponents;
 * launch(d_jobs, first, at, max_grid, kind, d_ext) starts jobs [first, at) of one kind.  h1_off (or null): where the
 * per-first-hand sums of record i begin (kind 2). */
template <class Launch>
static int exact_ext_stage(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n,
                           const std::vector<McqExactExtQuery> &xq, uint32_t n_kinds, uint64_t *h1_off, Launch launch) {
    const size_t job_bytes = (n * sizeof(McqExactExtJob) + 255u) & ~(size_t)255u;
    HIP_TRY(c->h_misc.reserve(job_bytes + n * sizeof(mcq_query_ext)));
    McqExactExtJob *jobs = static_cast<McqExactExtJob *>(c->h_misc.p);
    const McqExactExtJob *d_jobs = static_cast<const McqExactExtJob *>(c->h_misc.dev);
    memcpy(static_cast<uint8_t *>(c->h_misc.p) + job_bytes, ext, n * sizeof(mcq_query_ext));
    const uint32_t *d_ext = reinterpret_cast<const uint32_t *>(static_cast<uint8_t *>(c->h_misc.dev) + job_bytes);
    size_t at = 0;
    uint64_t off = 0;
    for (uint32_t kind = 0; kind < n_kinds; kind++) {
        const size_t first = at;
        uint32_t max_grid = 0;
        for (size_t i = 0; i < n; i++) {
            if (xq[i].b.n_opp != kind) continue;
            if (h1_off) h1_off[i] = off;
            const uint32_t g = mcq_exact_ext_plan(&q[i], (uint32_t)i, (uint32_t)i, kind, xq[i].b.L, (uint32_t)off,
                                                  exact_cu(c), &jobs[at++]);
            max_grid = g > max_grid ? g : max_grid;
            if (kind == 2u) off += (uint64_t)xq[i].n_rp * MCQ_XX_SUMS;
        }
        const int rc = launch(d_jobs, first, at, max_grid, kind, d_ext);
        if (rc) return rc;
    }
    return MCQ_OK;
}

/* mcq_exact_batch_ext, mcq_exact_batch_ext_ways, mcq_exact_batch_seats and mcq_exact_batch_ext_seats: rw = 64-bit words of
 * a weight row; prob -> mcq_exact_prob or mcq_exact_prob_ways (none for the per-seat rows), weights -> rows of rw words;
 * seat_opp = the random opponents a per-seat record may have (0: the all-in entry, 1: the extended one) */
static int exact_batch_ext_impl(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law, void *prob,
                                void *weights, uint32_t rw, const char *who, uint32_t seat_opp = 0u) {
    const bool ways = rw == kWaysWords, seats = rw == kSeatsWords;
    const size_t row_bytes = (size_t)rw * 8u;
    if (!c) return mcq_fail(MCQ_EINVAL, who, "null context");
    if (n == 0) return MCQ_OK;
    if (!q || !ext || (seats ? !weights : !prob)) return mcq_fail(MCQ_EINVAL, who, "null buffer");
    if (law != MCQ_LAW_REFERENCE && law != MCQ_LAW_UNIFORM) return mcq_fail(MCQ_EINVAL, who, "bad law");
    if (n > 65535u) return mcq_fail(MCQ_EINVAL, who, "at most 65535 queries per call");
    std::vector<McqExactExtQuery> xq;
    std::vector<uint8_t> rid;
    int rc = exact_ext_validate(
        q, ext, n, who,
        [law](const McqQueryWords &w, const McqExtRec &er, McqExactExtQuery &e) { return mcq_exact_ext_query(w, er, law, e); }, nullptr,
        [=](size_t, const McqExactExtQuery &e) -> const char * {
            if (seats && e.b.n_opp > seat_opp)
                return seat_opp == 0u ? "the per-seat enumeration takes known hands only (n_players == 1 + n_known)"
                                      : "two random opponents have no per-seat enumeration";
            if (e.b.n_opp == 2u && ways) return "two random opponents have no split-pot enumeration";
            return nullptr;
        },
        xq, rid);
    if (rc) return rc;
    uint64_t h1_words = 0; /* the per-first-hand sums of the two-opponent records */
    for (size_t i = 0; i < n; i++)
        if (xq[i].b.n_opp == 2u) h1_words += (uint64_t)xq[i].n_rp * MCQ_XX_SUMS;
    MCQ_ENTER(c, who);
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    HIP_TRY(c->d_res.reserve(n * row_bytes));
    c->res_clean = 0;
    HIP_TRY(c->h_res.reserve(n * row_bytes + h1_words * 8u));
    HIP_TRY(hipMemsetAsync(c->d_res.p, 0, n * row_bytes, c->stream));
    /* the per-first-hand sums of the two-opponent queries: the parity mode's draw buffer is free during this call */
    if (h1_words) {
        HIP_TRY(c->d_draws.reserve(h1_words * 8u));
        HIP_TRY(hipMemsetAsync(c->d_draws.p, 0, h1_words * 8u, c->stream));
    }
    std::vector<uint64_t> h1_off(n, 0);
    rc = exact_ext_stage(c, q, ext, n, xq, 3u, h1_off.data(),
                         [&](const McqExactExtJob *d_jobs, size_t first, size_t at, uint32_t max_grid, uint32_t kind, const uint32_t *d_ext) {
                             HIP_TRY(mcq_launch_exact_ext(d_jobs + first, (uint32_t)(at - first), max_grid, kind, d_ext, law, (mcq_result *)c->d_res.p,
                                                          (unsigned long long *)c->d_draws.p, c->d_luts, c->stream, ways, seats));
                             return (int)MCQ_OK;
                         });
    if (rc) return rc;
    uint8_t *hr = static_cast<uint8_t *>(c->h_res.p);
    HIP_TRY(hipMemcpyAsync(hr, c->d_res.p, n * row_bytes, hipMemcpyDeviceToHost, c->stream));
    if (h1_words)
        HIP_TRY(hipMemcpyAsync(hr + n * row_bytes, c->d_draws.p, h1_words * 8u, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (seats) { /* the rows are the result: integer weights, nothing to normalise */
        memcpy(weights, hr, n * row_bytes);
        return MCQ_OK;
    }
    const unsigned long long *h1 = reinterpret_cast<const unsigned long long *>(hr + n * row_bytes);
    for (size_t i = 0; i < n; i++) {
        mcq_result_ways w = {};
        memcpy(&w, hr + i * row_bytes, row_bytes);
        if (!ways) {
            mcq_exact_ext_finish(xq[i], &rid[64u * i], h1 + h1_off[i], w.r, static_cast<mcq_exact_prob *>(prob)[i]);
        } else { /* (at most one random opponent: one common total, the weights are always defined) */
            mcq_exact_prob_ways &pw = static_cast<mcq_exact_prob_ways *>(prob)[i];
            mcq_exact_ext_finish(xq[i], &rid[64u * i], h1, w.r, pw.p);
            for (uint32_t k = 0; k < 9u; k++) pw.tie_ways[k] = (double)w.tie_ways[k] / (double)w.r.runs;
        }
        if (weights) memcpy(static_cast<uint8_t *>(weights) + i * row_bytes, &w, row_bytes);
    }
    return MCQ_OK;
}

extern "C" {

int mcq_exact_batch_ext(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law, mcq_exact_prob *prob,
                        mcq_result *weights) {
    ABI_GUARD_BEGIN
    return exact_batch_ext_impl(c, q, ext, n, law, prob, weights, kPlainWords, "mcq_exact_batch_ext");
    ABI_GUARD_END("mcq_exact_batch_ext")
}

int mcq_exact_batch_ext_ways(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                             mcq_exact_prob_ways *prob, mcq_result_ways *weights) {
    ABI_GUARD_BEGIN
    return exact_batch_ext_impl(c, q, ext, n, law, prob, weights, kWaysWords, "mcq_exact_batch_ext_ways");
    ABI_GUARD_END("mcq_exact_batch_ext_ways")
}

int mcq_exact_batch_seats(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law, mcq_result_seats *weights) {
    ABI_GUARD_BEGIN
    return exact_batch_ext_impl(c, q, ext, n, law, nullptr, weights, kSeatsWords, "mcq_exact_batch_seats");
    ABI_GUARD_END("mcq_exact_batch_seats")
}

int mcq_exact_batch_ext_seats(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                              mcq_result_seats *weights) {
    ABI_GUARD_BEGIN
    return exact_batch_ext_impl(c, q, ext, n, law, nullptr, weights, kSeatsWords, "mcq_exact_batch_ext_seats", 1u);
    ABI_GUARD_END("mcq_exact_batch_ext_seats")
}

}  // extern "C"

/* every hero hand of a range against one random opponent from one enumeration per query (mcq_exact_hero.hpp).
 * preflop: the C(|D|, 5) completions go out in slices, several launches per call (mcq_exact_hero_pre.hpp).
 * weighted: opp_w (and hero_w, or null: every hand 1) hold a weight per hand, the law is the uniform one; before the flop the
 * opponent's range is then checked against every allowed hero hand BEFORE anything is launched. */
static int exact_hero_range_impl(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law, bool preflop,
                                 bool weighted, const uint16_t *opp_w, const uint16_t *hero_w, mcq_result *rows, mcq_exact_prob *agg,
                                 const char *who) {
    if (n == 0) return MCQ_OK; /* (nothing to do: not even a context is needed) */
    if (!c) return mcq_fail(MCQ_EINVAL, who, "null context");
    if (!q || !ext || !rows) return mcq_fail(MCQ_EINVAL, who, "null buffer");
    if (weighted && !opp_w) return mcq_fail(MCQ_EINVAL, who, "null opp_weights");
    if (law != MCQ_LAW_REFERENCE && law != MCQ_LAW_UNIFORM) return mcq_fail(MCQ_EINVAL, who, "bad law");
    if (preflop ? n > MCQ_HERO_PREFLOP_MAX_BATCH : n > MCQ_HERO_RANGE_MAX_BATCH)
        return mcq_fail(MCQ_EINVAL, who, preflop ? "at most MCQ_HERO_PREFLOP_MAX_BATCH queries per call"
                                                 : "at most MCQ_HERO_RANGE_MAX_BATCH queries per call");
    /* validation first: nothing is launched for a batch with one query that cannot be enumerated */
    std::vector<McqExactHeroQuery> xq(n);
    std::vector<uint8_t> rid(n * 64u);
    std::vector<uint16_t> hw_tab(weighted ? n * (size_t)MCQ_XP_MAX_PAIRS : 0u), ow_tab(weighted ? MCQ_XP_MAX_PAIRS : 0u);
    char buf[200];
    for (size_t i = 0; i < n; i++) {
        const McqExtRec er = {reinterpret_cast<const uint32_t *>(&ext[i])};
        int why = mcq_exact_hero_query(mcq_query_words(q[i]), er, law, !preflop, xq[i]);
        if (preflop && why == MCQ_XH_OK && q[i].n_board != 0) {
            snprintf(buf, sizeof buf, "query %zu: table cards: this entry enumerates before the flop only (n_board must be 0); "
                     "%s takes the flop, turn and river", i, weighted ? "mcq_exact_batch_hero_range_weighted" : "mcq_exact_batch_hero_range");
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
        if (why == MCQ_XH_OK) {
            const uint8_t *r_id = &rid[64u * i];
            uint16_t *hw = weighted ? &hw_tab[i * MCQ_XP_MAX_PAIRS] : nullptr;
            mcq_exact_ext_r_ids(xq[i].x, &rid[64u * i]);
            if (weighted)
                mcq_exact_hero_w_tables(xq[i], r_id, opp_w + i * MCQ_XH_ROWS, hero_w ? hero_w + i * MCQ_XH_ROWS : nullptr, 0u, 1u,
                                        ow_tab.data(), hw);
            xq[i].n_allowed = weighted ? mcq_exact_hero_count<true>(xq[i], r_id, hw, nullptr)
                                       : mcq_exact_hero_count<false>(xq[i], r_id, nullptr, nullptr);
            if (xq[i].n_allowed == 0u)
                why = MCQ_XH_EMPTY;
            /* exact before the flop (mcq_exact_hero_pre_w_undealable): the enumeration is not paid for to be thrown away */
            else if (preflop && weighted && mcq_exact_hero_pre_w_undealable(xq[i], ow_tab.data(), hw) != MCQ_XP_MAX_PAIRS)
                why = MCQ_XH_UNDEALABLE;
        }
        if (why != MCQ_XH_OK) {
            static const char *const reason[] = {
                "", "invalid extended query (as mcq_eval_batch_ext: distinct card ids < 52, at most 9 known hands, used ranges not empty)",
                "the hero is given as two cards (hero_is_range == 0): mcq_exact_batch_ext enumerates that",
                "known hands beside a hero range are not enumerated (n_known must be 0)",
                "a hero range is enumerated heads-up only (n_players must be 2)",
                "a hero range is enumerated postflop only (3 to 5 table cards): preflop every hero hand meets C(50, 5) table "
                "completions",
                "no hand of the hero's range can be made of the cards left",
                "the opponent's range cannot be dealt against some hand of the hero's range (no hand of positive weight shares no "
                "card with it)"};
            snprintf(buf, sizeof buf, "query %zu: %s%s", i, reason[why], weighted && why == MCQ_XH_EMPTY ? " with a positive weight" : "");
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
    }
    MCQ_ENTER(c, who);
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    const size_t q_bytes = (size_t)MCQ_XH_ROWS * sizeof(mcq_result);
    HIP_TRY(c->d_res.reserve(n * q_bytes));
    c->res_clean = 0;
    HIP_TRY(c->h_res.reserve(n * q_bytes));
    /* the rows are zeroed here postflop, where no plan fails; preflop only once every plan stands (below) */
    if (!preflop) HIP_TRY(hipMemsetAsync(c->d_res.p, 0, n * q_bytes, c->stream));
    /* jobs and extension records travel in pinned memory */
    const size_t job_bytes = (n * sizeof(McqExactExtJob) + 255u) & ~(size_t)255u;
    /* ... and behind them the weight tables: per query the opponent's, then the hero's (left out: never read) */
    const size_t ext_bytes = (n * sizeof(mcq_query_ext) + 255u) & ~(size_t)255u, w_bytes = 2u * MCQ_XH_ROWS * sizeof(uint16_t);
    HIP_TRY(c->h_misc.reserve(job_bytes + ext_bytes + (weighted ? n * w_bytes : 0u)));
    McqExactExtJob *jobs = static_cast<McqExactExtJob *>(c->h_misc.p);
    const McqExactExtJob *d_jobs = static_cast<const McqExactExtJob *>(c->h_misc.dev);
    memcpy(static_cast<uint8_t *>(c->h_misc.p) + job_bytes, ext, n * sizeof(mcq_query_ext));
    const uint32_t *d_ext = reinterpret_cast<const uint32_t *>(static_cast<uint8_t *>(c->h_misc.dev) + job_bytes);
    const uint16_t *d_wts = nullptr;
    if (weighted) {
        uint16_t *w = reinterpret_cast<uint16_t *>(static_cast<uint8_t *>(c->h_misc.p) + job_bytes + ext_bytes);
        for (size_t i = 0; i < n; i++) {
            memcpy(w + i * 2u * MCQ_XH_ROWS, opp_w + i * MCQ_XH_ROWS, w_bytes / 2u);
            if (hero_w) memcpy(w + (i * 2u + 1u) * MCQ_XH_ROWS, hero_w + i * MCQ_XH_ROWS, w_bytes / 2u);
        }
        d_wts = reinterpret_cast<const uint16_t *>(static_cast<uint8_t *>(c->h_misc.dev) + job_bytes + ext_bytes);
    }
    const uint32_t slice = mcq_exact_hero_pre_slice(c->hero_pre_slice); /* (preflop only) */
    uint32_t max_grid = 0, max_boards = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t g = mcq_exact_hero_plan(preflop, &q[i], (uint32_t)i, (uint32_t)i, xq[i].x.b.L, xq[i].n_allowed, exact_cu(c), slice,
                                               &jobs[i]);
        if (g == 0u) /* (preflop only) */
            return mcq_fail(MCQ_EINVAL, who, weighted ? "MCQ_HERO_PRE_SLICE: a launch would be longer than the plan allows"
                                                      : "MCQ_HERO_PRE_SLICE: a block would own more completions than its 32-bit sums allow");
        max_grid = g > max_grid ? g : max_grid;
        max_boards = jobs[i].n_boards > max_boards ? jobs[i].n_boards : max_boards;
    }
    if (preflop) HIP_TRY(hipMemsetAsync(c->d_res.p, 0, n * q_bytes, c->stream));
    /* postflop: one launch.  preflop: a launch per slice (a record with ghost cards has fewer completions: its blocks leave at once) */
    for (uint32_t lo = 0; lo < max_boards;) {
        const uint32_t hi = preflop && max_boards - lo > slice ? lo + slice : max_boards;
        HIP_TRY(mcq_launch_exact_hero(preflop, weighted, d_jobs, (uint32_t)n, max_grid, d_ext, law, d_wts, hero_w != nullptr, lo, hi,
                                      (mcq_result *)c->d_res.p, c->d_luts, c->stream));
        lo = hi;
    }
    HIP_TRY(hipMemcpyAsync(c->h_res.p, c->d_res.p, n * q_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* the aggregates first: a row without weight (the opponent's range cannot be dealt against that hero hand) refuses the
     * whole call before anything reaches the caller (preflop weighted: a backstop, the check above has seen it) */
    const mcq_result *hr = static_cast<const mcq_result *>(c->h_res.p);
    std::vector<mcq_exact_prob> p(n);
    for (size_t i = 0; i < n; i++)
        if (!mcq_exact_hero_finish(xq[i], &rid[64u * i], weighted ? &hw_tab[i * MCQ_XP_MAX_PAIRS] : nullptr, hr + i * MCQ_XH_ROWS, p[i])) {
            snprintf(buf, sizeof buf, "query %zu: the opponent's range cannot be dealt against some hand of the hero's range", i);
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
    memcpy(rows, hr, n * q_bytes);
    if (agg) memcpy(agg, p.data(), n * sizeof(mcq_exact_prob));
    return MCQ_OK;
}

extern "C" {

int mcq_exact_batch_hero_range(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law, mcq_result *rows,
                               mcq_exact_prob *agg) {
    ABI_GUARD_BEGIN
    return exact_hero_range_impl(c, q, ext, n, law, false, false, nullptr, nullptr, rows, agg, "mcq_exact_batch_hero_range");
    ABI_GUARD_END("mcq_exact_batch_hero_range")
}

/* ... with a weight per hand on both sides, under the uniform law */
int mcq_exact_batch_hero_range_weighted(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n,
                                        const uint16_t *opp_weights, const uint16_t *hero_weights, mcq_result *rows,
                                        mcq_exact_prob *agg) {
    ABI_GUARD_BEGIN
    return exact_hero_range_impl(c, q, ext, n, MCQ_LAW_UNIFORM, false, true, opp_weights, hero_weights, rows, agg,
                                 "mcq_exact_batch_hero_range_weighted");
    ABI_GUARD_END("mcq_exact_batch_hero_range_weighted")
}

/* ... before the flop */
int mcq_exact_batch_hero_range_preflop(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                       mcq_result *rows, mcq_exact_prob *agg) {
    ABI_GUARD_BEGIN
    return exact_hero_range_impl(c, q, ext, n, law, true, false, nullptr, nullptr, rows, agg, "mcq_exact_batch_hero_range_preflop");
    ABI_GUARD_END("mcq_exact_batch_hero_range_preflop")
}

/* ... before the flop with a weight per hand on both sides, under the uniform law */
int mcq_exact_batch_hero_range_preflop_weighted(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n,
                                                const uint16_t *opp_weights, const uint16_t *hero_weights, mcq_result *rows,
                                                mcq_exact_prob *agg) {
    ABI_GUARD_BEGIN
    return exact_hero_range_impl(c, q, ext, n, MCQ_LAW_UNIFORM, true, true, opp_weights, hero_weights, rows, agg,
                                 "mcq_exact_batch_hero_range_preflop_weighted");
    ABI_GUARD_END("mcq_exact_batch_hero_range_preflop_weighted")
}

/* flop and turn records, at most one random opponent: the weights row of every table completion (mcq_exact_runout.hpp) */
int mcq_exact_batch_ext_runouts(mcq_ctx *c, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                mcq_result_ways *cards, mcq_result_ways *pairs) {
    ABI_GUARD_BEGIN
    const char *who = "mcq_exact_batch_ext_runouts";
    if (n == 0) return MCQ_OK; /* (nothing to do: not even a context is needed) */
    if (!c) return mcq_fail(MCQ_EINVAL, who, "null context");
    if (!q || !ext || !cards) return mcq_fail(MCQ_EINVAL, who, "null buffer");
    if (law != MCQ_LAW_REFERENCE && law != MCQ_LAW_UNIFORM) return mcq_fail(MCQ_EINVAL, who, "bad law");
    if (n > MCQ_RUNOUT_MAX_BATCH) return mcq_fail(MCQ_EINVAL, who, "at most MCQ_RUNOUT_MAX_BATCH queries per call");
    static const char *const more[] = {
        "two random opponents have no split-pot enumeration, so none per runout",
        "runouts are enumerated on the flop and the turn only (3 or 4 table cards): preflop a record has C(50, 5) "
        "completions",
        "five table cards: no card to come"};
    std::vector<McqExactExtQuery> xq;
    std::vector<uint8_t> rid;
    int rc = exact_ext_validate(
        q, ext, n, who,
        [law](const McqQueryWords &w, const McqExtRec &er, McqExactExtQuery &e) { return mcq_exact_runout_query(w, er, law, e); }, more,
        [](size_t, const McqExactExtQuery &) -> const char * { return nullptr; }, xq, rid);
    if (rc) return rc;
    MCQ_ENTER(c, who);
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    /* device rows: the card rows of all records, then their pair rows -- each part is handed back with one copy */
    const size_t card_bytes = n * MCQ_XR_CARD_ROWS * sizeof(mcq_result_ways), pair_bytes = n * MCQ_XR_PAIR_ROWS * sizeof(mcq_result_ways);
    const size_t back_bytes = card_bytes + (pairs ? pair_bytes : 0u);
    HIP_TRY(c->d_res.reserve(card_bytes + pair_bytes));
    c->res_clean = 0;
    HIP_TRY(c->h_res.reserve(back_bytes));
    HIP_TRY(hipMemsetAsync(c->d_res.p, 0, card_bytes + pair_bytes, c->stream));
    mcq_result_ways *d_cards = static_cast<mcq_result_ways *>(c->d_res.p), *d_pairs = d_cards + n * MCQ_XR_CARD_ROWS;
    rc = exact_ext_stage(c, q, ext, n, xq, 2u, nullptr,
                         [&](const McqExactExtJob *d_jobs, size_t first, size_t at, uint32_t max_grid, uint32_t kind, const uint32_t *d_ext) {
                             HIP_TRY(mcq_launch_exact_runouts(d_jobs + first, (uint32_t)(at - first), max_grid, kind, d_ext, law, d_cards, d_pairs,
                                                              c->d_luts, c->stream));
                             return (int)MCQ_OK;
                         });
    if (rc) return rc;
    const McqExactExtJob *d_jobs = static_cast<const McqExactExtJob *>(c->h_misc.dev);
    HIP_TRY(mcq_launch_exact_runout_cards(d_jobs, (uint32_t)n, d_cards, d_pairs, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_res.p, c->d_res.p, back_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(cards, c->h_res.p, card_bytes);
    if (pairs) memcpy(pairs, static_cast<const uint8_t *>(c->h_res.p) + card_bytes, pair_bytes);
    return MCQ_OK;
    ABI_GUARD_END("mcq_exact_batch_ext_runouts")
}

}  // extern "C"

/* mcq_exact_matrix and mcq_exact_matrix_device (mcq_exact_matrix.hpp): one implementation.  The batch goes out in chunks of at
 * most c->matrix_chunk records, three launches each on stream s; a record's scratch -- key table and counts by D-pair -- is
 * one of the chunk's slots in the stream's scratch buffer, all slots sized for the largest record of the batch (the sizes
 * change nothing in the output: every word a kernel reads was written for that record by the launch before).  d_win / d_tie:
 * the caller's device matrices, or null: the host entry, whose chunks land in c->d_res and travel back through pinned memory. */
static int exact_matrix_impl(mcq_ctx *c, const mcq_matrix_query *q, size_t n, uint16_t *h_win, uint16_t *h_tie, uint16_t *d_win,
                             uint16_t *d_tie, uint32_t *total, hipStream_t user_stream, const char *who) {
    const bool host = d_win == nullptr;
    if (!c) return mcq_fail(MCQ_EINVAL, who, "null context");
    if (n == 0) return mcq_fail(MCQ_EINVAL, who, "no record (n == 0)");
    if (n > MCQ_MATRIX_MAX_BATCH) return mcq_fail(MCQ_EINVAL, who, "at most MCQ_MATRIX_MAX_BATCH records per call");
    if (!q) return mcq_fail(MCQ_EINVAL, who, "null records");
    if (host && !h_win) return mcq_fail(MCQ_EINVAL, who, "null win");
    /* validation first: nothing is launched for a batch with one record that is refused */
    std::vector<McqMatrixJob> jobs(n);
    std::vector<uint32_t> tot(n);
    uint32_t max_stride = 0, max_stages = 0;
    for (size_t i = 0; i < n; i++) {
        static const char *const reason[] = {
            "",
            "the matrix is enumerated on the flop, the turn and the river (n_board 3 to 5): preflop it is C(48, 5) completions "
            "per pair with 32-bit counts",
            "reserved bytes must be 0",
            "bits 52..63 of the dead mask must be 0",
            "a table card id is not below 52",
            "a table card is given twice",
            "a table card is also dead",
            "too few cards left: no two hands leave a table completion (L - 4 < k)"};
        McqMatrixQuery e;
        const int why = mcq_matrix_query_build(q[i], e);
        if (why != MCQ_XM_OK) {
            char buf[200];
            snprintf(buf, sizeof buf, "record %zu: %s", i, reason[why]);
            return mcq_fail(MCQ_EINVAL, who, buf);
        }
        jobs[i].q = q[i];
        jobs[i].stride = mcq_matrix_stride(e.n_rp);
        jobs[i].stages = mcq_matrix_stages(e.n_boards);
        tot[i] = e.total;
        max_stride = jobs[i].stride > max_stride ? jobs[i].stride : max_stride;
        max_stages = jobs[i].stages > max_stages ? jobs[i].stages : max_stages;
    }
    MCQ_ENTER(c, who);
    McqDeviceScope dev_(c->device);
    HIP_TRY(dev_.err);
    hipStream_t s = host ? c->stream : user_stream;
    if (!host && stream_capturing(s)) return mcq_fail(MCQ_EINVAL, who, "the stream is being captured: this entry is not captured into a graph");
    uint32_t chunk = c->matrix_chunk < MCQ_XM_MAX_CHUNK ? c->matrix_chunk : MCQ_XM_MAX_CHUNK;
    chunk = chunk < 1u ? 1u : chunk > n ? (uint32_t)n : chunk;
    const size_t key_words = (size_t)max_stages * MCQ_XM_STAGE * max_stride, cnt_words = (size_t)max_stride * max_stride;
    const size_t key_bytes = chunk * key_words * sizeof(uint32_t), mat = (size_t)MCQ_XH_ROWS * MCQ_XH_ROWS, mat_bytes = mat * sizeof(uint16_t);
    mcq_ctx::Scratch *sc = nullptr;
    const int rc = scratch_for(c, s, key_bytes + chunk * cnt_words * sizeof(uint16_t), false, &sc);
    if (rc) return rc;
    uint32_t *d_keys = static_cast<uint32_t *>(sc->prefix.p);
    uint16_t *d_cnt = reinterpret_cast<uint16_t *>(static_cast<uint8_t *>(sc->prefix.p) + key_bytes);
    const size_t mats = h_tie || d_tie ? 2u : 1u;
    if (host) {
        HIP_TRY(c->d_res.reserve(chunk * mats * mat_bytes));
        c->res_clean = 0;
        HIP_TRY(c->h_res.reserve(chunk * mats * mat_bytes));
        d_win = static_cast<uint16_t *>(c->d_res.p);
        d_tie = h_tie ? d_win + chunk * mat : nullptr;
    }
    if (total) memcpy(total, tot.data(), n * sizeof(uint32_t));
    const bool timed = c->timing;
    const uint64_t timed0 = c->n_timed;
    c->last_ms = 0.f;
    for (size_t a = 0; a < n; a += chunk) {
        const uint32_t m = (uint32_t)(n - a < chunk ? n - a : chunk);
        uint32_t stride = 0, stages = 0;
        for (uint32_t i = 0; i < m; i++) {
            jobs[a + i].slot = i;
            jobs[a + i].out = host ? i : (uint32_t)(a + i);
            stride = jobs[a + i].stride > stride ? jobs[a + i].stride : stride;
            stages = jobs[a + i].stages > stages ? jobs[a + i].stages : stages;
        }
        /* the grids by the CUs the plans may see, shared among the chunk's records: one block walks everything under MCQ_EXACT_CU=1 */
        const uint32_t cu = exact_cu(c), per = cu / m < 1u ? 1u : cu / m, rows = stages * MCQ_XM_STAGE;
        const uint32_t rank_grid = per < rows ? per : rows, finish_grid = 4u * per < MCQ_XH_ROWS ? 4u * per : MCQ_XH_ROWS;
        hipEvent_t ev[6];
        for (int k = 0; k < 3; k++) {
            const int slot = (int)((c->n_timed + (uint64_t)k) % mcq_ctx::kRing);
            ev[2 * k] = c->ev0[slot];
            ev[2 * k + 1] = c->ev1[slot];
        }
        HIP_TRY(mcq_launch_exact_matrix(&jobs[a], m, rank_grid, finish_grid, stride, d_keys, key_words, d_cnt, cnt_words, d_win, d_tie,
                                        c->d_luts, s, timed ? ev : nullptr));
        if (timed) c->n_timed += 3u;
        if (host) {
            uint8_t *back = static_cast<uint8_t *>(c->h_res.p);
            HIP_TRY(hipMemcpyAsync(back, d_win, m * mat_bytes, hipMemcpyDeviceToHost, s));
            if (h_tie) HIP_TRY(hipMemcpyAsync(back + chunk * mat_bytes, d_tie, m * mat_bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            memcpy(h_win + a * mat, back, m * mat_bytes);
            if (h_tie) memcpy(h_tie + a * mat, back + chunk * mat_bytes, m * mat_bytes);
        }
    }
    /* a caller's stream may run on while another stream's call takes over the scratch: mark its last reader */
    if (sc != &c->scratch[0]) {
        HIP_TRY(hipEventRecord(sc->done, s));
        sc->done_recorded = true;
    }
    if (host && timed) { /* the kernels of this call, as far as the ring of events still holds them */
        float ms[mcq_ctx::kRing];
        const uint64_t launched = c->n_timed - timed0;
        const int want = (int)(launched < (uint64_t)mcq_ctx::kRing ? launched : (uint64_t)mcq_ctx::kRing);
        const int got = kernel_times_impl(c, ms, want);
        for (int k = 0; k < got; k++) c->last_ms += ms[k];
    }
    return MCQ_OK;
}

extern "C" {

int mcq_exact_matrix(mcq_ctx *c, const mcq_matrix_query *q, size_t n, uint16_t *win, uint16_t *tie, uint32_t *total) {
    ABI_GUARD_BEGIN
    return exact_matrix_impl(c, q, n, win, tie, nullptr, nullptr, total, nullptr, "mcq_exact_matrix");
    ABI_GUARD_END("mcq_exact_matrix")
}

int mcq_exact_matrix_device(mcq_ctx *c, const mcq_matrix_query *q, size_t n, void *d_win, void *d_tie, uint32_t *total,
                            void *hip_stream) {
    ABI_GUARD_BEGIN
    if (!d_win) return mcq_fail(MCQ_EINVAL, "mcq_exact_matrix_device", "null win");
    return exact_matrix_impl(c, q, n, nullptr, nullptr, static_cast<uint16_t *>(d_win), static_cast<uint16_t *>(d_tie), total,
                             (hipStream_t)hip_stream, "mcq_exact_matrix_device");
    ABI_GUARD_END("mcq_exact_matrix_device")
}

}  // extern "C"
