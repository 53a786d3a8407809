/*
 * gossiphip.h — C-ABI of libgossiphip, the MI355X-native batched
 * gossip-membership / failure-detection / replica-placement engine.
 *
 * This is the drop-in boundary for the hot path of
 * xiaoxin0515/P2P-File-system-with-Gossip-Detect-Failure-Management
 * (SURVEY.md §8b). The reference has no FFI; its hot path sits behind Go
 * methods and a net/rpc service. Each entry point below names the reference
 * interface it replaces (file:line under the reference tree). Semantics:
 * SPEC.md. Host bindings: INTEGRATION.md (cgo stub) and
 * p2p-file-system-with-gossip-detect-failure-management_amd/gossipsim (ctypes).
 *
 * Conventions
 *   - Every function returns 0 (GH_OK) or a negative GH_E* code; the reason is
 *     in gh_last_error(h). The reference instead log.Fatal/log.Panic's
 *     (slave/slave.go:214,262-270; master/master.go:130-135).
 *   - Buffers are caller-owned host memory, read or written only during the
 *     call. The handle owns all device memory (HBM) and the HIP stream.
 *   - A handle is not thread-safe (call it from one thread; cgo callers use
 *     runtime.LockOSThread).
 *   - Member IDs are dense int32 in [0, n_members); file IDs dense int32 in
 *     [0, max_files).
 *   - There is no CPU fallback: gh_create fails with GH_ENODEV when no gfx950
 *     device is usable.
 */
#ifndef GOSSIPHIP_H_
#define GOSSIPHIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GH_ABI_VERSION 8

/* ---- error codes ---------------------------------------------------- */
#define GH_OK 0
#define GH_EINVAL (-1)               /* bad argument / shape                    */
#define GH_ENODEV (-2)               /* no usable HIP device                    */
#define GH_ENOMEM (-3)               /* device allocation failed / wide arena full */
#define GH_EHIP (-4)                 /* HIP runtime error                       */
#define GH_EPLACEMENT_STARVED (-5)   /* master/master.go:130-135 hang / panic   */
#define GH_ERANGE (-6)               /* heartbeat would pass INT32_MAX / < range */

/* ---- cell encoding (SPEC.md §1) -------------------------------------- */
#define GH_ABSENT (-1)     /* not in MemberList                              */
#define GH_TOMBSTONE (-2)  /* in RecentFailList (slave/slave.go:65)          */

/* ---- modes ------------------------------------------------------------ */
#define GH_PEER_PULL 0     /* receiver pulls k Philox-selected peers          */
#define GH_PEER_RING 1     /* reference ring push, slave/slave.go:512-524     */
#define GH_DETECT_CANONICAL 0
#define GH_DETECT_QUIRK 1  /* Go range-over-mutated-slice skip, slave.go:464   */
/* MemberList order (SPEC.md §7 D1). GH_ORDER_ID keeps every list in member-ID
 * order: pull mode with canonical detection is order-free (the benched
 * configurations), and it needs no per-row order state. GH_ORDER_APPEND keeps
 * the reference's slice order: members are appended when added
 * (slave/slave.go:255 addNewMember, :437 MergeMemberList, in received-list
 * order, senders in ID order) and keep their relative order when others are
 * removed (:283); ring targets (:515-524), quirk runs (:464-477),
 * MemberList[0] (:936, :994), placement candidates (master/master.go:46,
 * :135) and lsm follow it. One engine or row shards (GH_LAYOUT_ROWS: every
 * shard keeps every row's list, the owners' changes are copied each round);
 * column shards refuse it (gh_create_sharded: GH_EINVAL). HBM +8*N*N bytes
 * per engine / shard (double-buffered [N][N] int32 lists); row shards also
 * keep the list copy's scratch, grown to (G + 1) x 256 MiB at most (the
 * changed lists travel in ranges of 2^26 / N rows). */
#define GH_ORDER_ID 0
#define GH_ORDER_APPEND 1
/* Who receives a detector's REMOVE (SPEC D4). GH_REMOVE_LIST is the
 * reference: Remove (slave/slave.go:338-363) runs right after removeMember
 * inside the detection sweep (:472-473) and messages every member of the
 * detector's list as it stands then (the member itself and the members the
 * sweep removed before it are gone, the later ones still listed), itself
 * excluded (:344-346). GH_REMOVE_ALL delivers it to every alive row but a sole
 * detector (equal whenever the detectors' lists agree, as in a healthy
 * cluster; the victim of a false positive then removes itself too). */
#define GH_REMOVE_ALL 0
#define GH_REMOVE_LIST 1

/* ---- events (SPEC.md §5) ---------------------------------------------- */
#define GH_EV_JOIN 1       /* slave/slave.go:288 Join + :250 addNewMember     */
#define GH_EV_LEAVE 2      /* slave/slave.go:310 Leave                        */
#define GH_EV_CRASH 3      /* README.md:30 "CTRL+C to crash node"            */

typedef struct gh_config {
  int32_t n_members;     /* N; member IDs 0..N-1                             */
  int32_t fanout;        /* k (pull mode), 1..8                              */
                         /* k = 3..4 take the sender plane and the 4-bit tier
                          * (slower dissemination, k < 3, leaves views outside
                          * the plane's window); k >= 5 takes the 8-sender
                          * round kernel (k_round<KB = 8>, k <= 4: KB = 4)     */
  int32_t peer_mode;     /* GH_PEER_PULL | GH_PEER_RING                      */
  int32_t detect_mode;   /* GH_DETECT_CANONICAL | GH_DETECT_QUIRK            */
  int32_t t_fail;        /* PERIOD in rounds, slave/slave.go:24 (5)          */
  int32_t t_cleanup;     /* COOLDOWN in rounds, slave/slave.go:25 (5)        */
  int32_t min_members;   /* literal 4, slave/slave.go:504,511                */
  int32_t replicas;      /* 4, master/master.go:131 (1..8)                   */
  int32_t introducer;    /* INTRODUCER_ADDR, slave/slave.go:22 (0)           */
  int32_t master;        /* master row whose list is Member_list (0)        */
  int32_t device;        /* HIP device ordinal                               */
  int32_t tile_width;    /* HBM layout: members per table tile (8, 16, 32,
                            64, 128 or 256, anything else GH_EINVAL; 0 =
                            default: 64, 256 with the sender plane), see
                            DESIGN.md; gh_debug_knobs reports it            */
  uint64_t seed;         /* Philox key for peers and placement draws         */
  int64_t max_files;     /* file-metadata capacity (0 = no files)            */
  int64_t wide_segments; /* slots of each wide-segment arena (HBM layout,
                            DESIGN.md); 0 = auto (all segments when small,
                            else 1/32 of them, grown between calls)        */
  int32_t shard_layout;  /* sharded engines (gh_create_sharded):
                            GH_LAYOUT_COLUMNS (0, default) or GH_LAYOUT_ROWS */
  int32_t list_order;    /* GH_ORDER_ID (0, default) or GH_ORDER_APPEND      */
  int32_t remove_mode;   /* REMOVE recipients: GH_REMOVE_ALL (0, default) or
                            GH_REMOVE_LIST (the reference's, slave.go:344)  */
  int32_t reserved[3];
} gh_config;

typedef struct gh_event {
  int32_t kind;          /* GH_EV_*                                          */
  int32_t member;
} gh_event;

/* Counters accumulated over the rounds of one gh_step call. */
typedef struct gh_round_stats {
  int64_t rounds;         /* rounds executed by this call                    */
  int64_t last_round;     /* `now` of the last round executed                */
  int64_t detections;     /* cells removed by detectfailure (slave.go:472)   */
  int64_t failed_members; /* Σ_rounds distinct members detected that round   */
  int64_t remove_unknown; /* REMOVE/LEAVE of an unknown member (slave.go:280 panic) */
  int64_t ring_empty;     /* ring sender with empty list (slave.go:517 div-by-0)   */
  int64_t active_rows;    /* Σ_rounds rows passing the <4 guard              */
  int64_t merged_cells;   /* cells advanced or added by MergeMemberList      */
  int64_t released;       /* tombstones dropped by cleanFailList             */
  int64_t tombstoned;     /* tombstones created by REMOVE/LEAVE delivery     */
} gh_round_stats;

/* One re-replication plan entry (master/master.go:27-31 Replicate_info). */
typedef struct gh_plan_entry {
  int32_t file;
  int32_t node1;          /* first working replica, -1 if none (SPEC D5)     */
  int32_t version;
  int32_t n_new;
  int32_t status;         /* GH_OK or GH_EPLACEMENT_STARVED                  */
  int32_t new_nodes[8];   /* first n_new valid                               */
} gh_plan_entry;

/* Fills *cfg with the reference defaults (SURVEY.md §5 Config). */
void gh_config_default(gh_config* cfg);

/* Replaces InitSlave/InitMaster (slave/slave.go:95, master/master.go:38) for
 * N members at once. HBM: the 16-bit narrow table (x2), 4*N*N bytes; in pull
 * mode with 3 <= k <= 4 from N = 16,384 the sender plane (x2, N*N bytes) and
 * the 4-bit tier's age plane (x2, N*N bytes); plus the wide-segment arenas
 * (gh_config.wide_segments) and a frozen store for stopped rows that grows
 * with them (gh_memory_info). */
int gh_create(const gh_config* cfg, void** handle);
void gh_destroy(void* h);
const char* gh_last_error(void* h);
int gh_abi_version(void);

/* Whole-state transfer (host <-> HBM). Rows [row0, row0+n_rows) of the N x N
 * tables. `round` is the tick of the last completed round. hb: any int32
 * >= -2 (GH_ABSENT, GH_TOMBSTONE, heartbeats up to INT32_MAX; below -2 is
 * GH_ERANGE); ts: any int32. Pending REMOVEs are cleared on import. Export:
 * the ts of an absent cell is 0 (the reference keeps no entry for it), and
 * with T_cleanup < 30 a tombstone older than T_cleanup + 1 rounds exports
 * ts = round + 1 - (T_cleanup + 1) (its age is only ever compared with
 * COOLDOWN, slave/slave.go:490; SPEC.md §1). */
int gh_import_state(void* h, const int32_t* hb, const int32_t* ts,
                    const uint8_t* alive, int64_t row0, int64_t n_rows,
                    int32_t round);
int gh_export_state(void* h, int32_t* hb, int32_t* ts, uint8_t* alive,
                    int64_t row0, int64_t n_rows);
/* Every row alive and holding every member at (hb0, ts0): the synthetic
 * full-membership start of BASELINE configs 2-4, filled on the device. */
int gh_init_full(void* h, int32_t hb0, int32_t ts0, int32_t round);
int gh_get_round(void* h, int32_t* round);

/* Queue churn for the next round (GetMsg JOIN/LEAVE dispatch,
 * slave/slave.go:224-240; crash = process death). */
int gh_apply_events(void* h, const gh_event* ev, int64_t n);

/* Run `rounds` synchronous gossip rounds (HeartBeat, slave/slave.go:499,
 * driven by the 1 s loop of main.go:27-33, with MergeMemberList :414,
 * detectfailure :460, cleanFailList :484). Blocks until done; stats may be
 * NULL. Heartbeats are Go ints in the reference (master/master.go:18) and
 * int32 here: a round in which a running member's own heartbeat is
 * INT32_MAX is refused with GH_ERANGE (the rounds before it completed;
 * stats->rounds says how many). GH_ENOMEM: the wide arena overflowed inside
 * a round and the state is lost (re-import or destroy). */
int gh_step(void* h, int32_t rounds, gh_round_stats* stats);

/* Members detected in the last round as an N-bit bitmap (REMOVE broadcast
 * set, slave/slave.go:338). */
int gh_read_failed(void* h, uint32_t* bitmap, int64_t n_words);
/* Rows that detected a failure in the last round (they call Fail_recover,
 * slave/slave.go:479-481). Returns the count via *n_out (<= cap written). */
int gh_read_detectors(void* h, int32_t* rows, int64_t cap, int64_t* n_out);
/* "lsm" (slave/slave.go:558-561): observer's present members, in list order
 * (member-ID order under GH_ORDER_ID). */
int gh_lsm(void* h, int32_t observer, int32_t* ids, int32_t* hb, int32_t* ts,
           int64_t cap, int64_t* n_out);
/* Membership census: per member column, how the running rows see it, and the
 * age distribution of every view, reduced on the device in one read-only pass
 * over the table (no reference counterpart; the nearest is running `lsm`,
 * slave/slave.go:558-561, on every VM). Defined on what gh_export_state
 * would return now (hb, ts, alive; R = gh_get_round; queued events and the D7
 * shadow entries are not in it): for member c, S_c = the rows i != c with
 * alive[i] and hb[i][c] >= 0, T_c = those with hb[i][c] == GH_TOMBSTONE, and
 * age(i, c) = max(0, R + 1 - ts[i][c]) (SPEC §3, at most INT32_MAX). A
 * member's own entry is in neither, as in the detector (SPEC §2 step 4).
 *   listed[c] = |S_c|, tombstoned[c] = |T_c|;
 *   hb_min[c], hb_max[c] = min / max of hb[i][c] over S_c, hb_sum[c] their sum
 *     (mean lag = hb_max - hb_sum / listed), age_max[c] = max age(i, c) over
 *     S_c; an empty S_c gives -1, -1, 0, -1;
 *   age_hist[b], b < GH_CENSUS_BINS = the (i, c), i in S_c, with
 *     min(age(i, c), GH_CENSUS_BINS - 1) == b: the sum over b > T_fail is the
 *     number of step-4 candidates of the next round.
 * Outputs: [N] each by member id, age_hist [GH_CENSUS_BINS]; any may be NULL.
 * Additive under ABI 7. On a sharded handle the call is collective: every
 * rank calls it, and every rank gets the global result. */
#define GH_CENSUS_BINS 32
int gh_census(void* h, int32_t* listed, int32_t* tombstoned, int32_t* hb_min,
              int32_t* hb_max, int64_t* hb_sum, int32_t* age_max, int64_t* age_hist);

/* Membership groups and view digests: which clusters the running members'
 * lists now form, and which running members hold the same view, computed on
 * the device by read-only passes over the table (no reference counterpart;
 * the nearest is comparing the `lsm` of every VM, slave/slave.go:558-561).
 * Defined on what gh_export_state would return now (hb, alive; as for
 * gh_census, queued events and the D7 shadow entries are not in it).
 *   Edges: E = {(i, c) : i != c, alive[i], alive[c], hb[i][c] >= 0}, "running
 *   i lists running c". A stopped member has no edges: nothing bridges through
 *   a stopped member two groups both still list, nor through a stopped row's
 *   stale list. Tombstones and absent cells are no edge.
 *   group[m], m running = the lowest member id of m's weakly connected
 *   component of (running members, E), direction ignored; m stopped: -1. A
 *   running member nobody lists and that lists nobody is its own group. Weak,
 *   because one listing in either direction lets gossip -- and with it the
 *   missing entries -- flow (a pull from a peer that lists the receiver, a
 *   ring target taken from the sender's list): two different groups never
 *   hear from each other again except through a JOIN, which is the "never
 *   re-merge" statement of gh_set_partition below.
 *   view_digest[i], i running = the sum modulo 2^64 of mix(c) over every c
 *   with hb[i][c] >= 0, the row's own entry and the stopped members it still
 *   lists included; i stopped: 0. mix(c), in uint64:
 *     z = (c + 1) * 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31.
 *   Equal views give equal digests, so the distinct digests among the running
 *   rows count the distinct views; two different views collide with
 *   probability about 2^-64.
 *   *n_groups = the running m with group[m] == m. *passes = the hooking
 *   passes the call ran (>= 1; diagnostic, it may differ between engines that
 *   hold the same state).
 * group, view_digest: [N] by member id. Any output may be NULL, both arrays
 * included (the counts are still returned; without view_digest no digest is
 * computed). A NULL handle returns GH_EINVAL before any device is touched.
 * Read-only: the table, the round, the statistics, the draw counters and
 * every diagnostic are unchanged. Each pass reads the table once (what a
 * gh_census reads); labels are member ids that only decrease, so the passes
 * end: two on a healthy cluster, two or three on the split and shattered
 * states measured in DESIGN.md "Groups". Nothing is allocated or launched before the first call
 * (gh_footprint, gh_memory_info at creation and gh_step's launches do not
 * change); the first call allocates 20 N + 16 bytes of scratch per shard,
 * kept until gh_destroy. Any engine: both peer modes, detection modes, list
 * orders and remove modes, armed or not, loss and journal on or off.
 * Additive under ABI 7. On a sharded handle (either layout) the call is
 * collective: every rank calls it with the same outputs NULL and gets the
 * global result. */
int gh_groups(void* h, int32_t* group, uint64_t* view_digest, int64_t* n_groups,
              int32_t* passes);

/* Detection journal: what a failure detector is judged by -- how long a crash
 * takes to be detected, how often a running member is declared dead, how long
 * the verdict takes to reach every view -- kept on the device and updated once
 * per round inside gh_step by one O(N) kernel, read out on demand (no
 * reference counterpart: the reference only logs each detection,
 * detectfailure slave/slave.go:460-482, and each REMOVE it sends, Remove
 * :338-363). Off by default: gh_step then launches and allocates nothing new,
 * and gh_create's allocations and gh_footprint do not include it.
 * gh_journal_enable: mode GH_JOURNAL_OFF / DETECT / VIEWS (any other:
 * GH_EINVAL), log_rounds in 0..2^20 (else GH_EINVAL) = the rounds the log ring
 * keeps. Every call clears the journal (re-enabling restarts it); a non-off
 * mode allocates it and takes the current alive[] as the baseline.
 * gh_import_state and gh_init_full clear it too and take the new alive[]. It
 * persists across gh_step calls; a round a call did not run (GH_ERANGE) is
 * not journaled.
 *   For a journaled round r, after the round: a[c] = alive[c] as the round ran
 *   (after its events), pa[c] = a[c] of the previous journaled round or the
 *   baseline, cnt[c] / dmin[c] = the rows that detected member c in round r
 *   (the cells detectfailure removed, slave/slave.go:472) and the lowest of
 *   them, running = sum of a. Per member c, in this order:
 *   1. a && !pa: start_round = r, stop_round = -1. !a && pa: stop_round = r.
 *      Either resets the phase: first_round = first_detector = -1,
 *      first_count = 0, forgotten_round = known_round = -1. Fields never set
 *      are -1 (a member stopped before the baseline keeps stop_round = -1).
 *   2. cnt > 0: det_rounds++, detectors += cnt, last_round = r; if a (a false
 *      positive) fp_rounds++. If first_round < 0: first_round = r,
 *      first_detector = dmin, first_count = cnt, and if !a && stop_round >= 0
 *      latency_hist[min(r - stop_round, GH_JOURNAL_BINS - 1)]++: the detection
 *      latency, once per stop.
 *   3. GH_JOURNAL_VIEWS only, L = gh_census's listed[c] of the table after
 *      round r: !a && forgotten_round < 0 && L == 0: forgotten_round = r, and
 *      if stop_round >= 0 forget_hist[min(r - stop_round, BINS - 1)]++;
 *      a && known_round < 0 && L == running - 1: known_round = r, and if
 *      start_round >= 0 known_hist[min(r - start_round, BINS - 1)]++. In
 *      DETECT mode both fields stay -1 and both histograms 0.
 *   The round's log entry (gh_journal_round): round = r, running; failed =
 *   |D_r| (gh_round_stats.failed_members of that round), false_failed = the
 *   running members among them; detections = sum of cnt (gh_round_stats.
 *   detections of that round), false_detections = that over the running
 *   members; stale_views = sum of L over the stopped members, missing_views =
 *   sum of (running - 1 - L) over the running ones (both -1 without VIEWS).
 * gh_journal_read: per-member outputs [N] by member id, the histograms
 * [GH_JOURNAL_BINS]; any output may be NULL. gh_journal_rounds: the log is a
 * ring of the last log_rounds rounds; *n_total = the rounds journaled since
 * enable, the newest *n_out = min(*n_total, log_rounds, cap) entries are
 * written, oldest first (n_total, n_out may be NULL; out may be NULL with
 * cap 0). With the journal off both return GH_EINVAL; a NULL handle returns
 * GH_EINVAL from all three before any device is touched. Cost per round, at
 * N = 65,536, k = 4 on a MI355X (DESIGN.md "Journal"): DETECT one O(N) launch,
 * 8.5 us beside a 2.14 ms round; VIEWS adds one census pass over the table per
 * round, 1.60 ms: a round then takes 1.74 times as long.
 * Additive under ABI 7. On a sharded handle all three calls are collective:
 * every rank calls them with the same arguments (the same outputs NULL), and
 * every rank gets the global result. */
#define GH_JOURNAL_OFF 0
#define GH_JOURNAL_DETECT 1   /* detections, false positives, latency          */
#define GH_JOURNAL_VIEWS 3    /* DETECT + dissemination: one census pass/round */
#define GH_JOURNAL_BINS 64
typedef struct gh_journal_round {      /* 48 bytes */
  int32_t round, running, failed, false_failed;
  int64_t detections, false_detections, stale_views, missing_views;
} gh_journal_round;
int gh_journal_enable(void* h, int32_t mode, int64_t log_rounds);
int gh_journal_read(void* h, int32_t* stop_round, int32_t* start_round,
                    int32_t* first_round, int32_t* first_detector, int32_t* first_count,
                    int32_t* last_round, int32_t* det_rounds, int64_t* detectors,
                    int32_t* fp_rounds, int32_t* forgotten_round, int32_t* known_round,
                    int64_t* latency_hist, int64_t* forget_hist, int64_t* known_hist);
int gh_journal_rounds(void* h, gh_journal_round* out, int64_t cap,
                      int64_t* n_total, int64_t* n_out);

/* Lossy gossip links: per-member send / receive drop rates of the gossip
 * messages. They model the one transport of the reference that loses
 * messages, the UDP datagrams a member's list travels in (slave/slave.go:
 * 527-542); JOIN, LEAVE and REMOVE stay reliable unless gh_set_control_loss
 * (below) opts them in; gh_merge_list always is (SPEC D9).
 * State: thresholds in units of 2^-32, out[m] for member m's sends and in[m]
 * for its receives. hit(thr, w) = thr == GH_LOSS_ALWAYS || w < thr: 0
 * (GH_LOSS_NEVER) never drops, GH_LOSS_ALWAYS always does. B(a, r, blk) = the
 * Philox4x32-10 block of counter (a, r, 'LINK' = 0x4C494E4B, blk) under the
 * engine's seed; r = the round being run (SPEC §2 step 6a).
 *   Pull mode: receiver i's draw t < k of peer p, drawn exactly as without
 *   loss, is a message iff it is valid without loss (p alive and active, i in
 *   p's snapshot list and not REMOVE'd at p). The message is dropped iff
 *   hit(out[p], B(i, r, t)[0]) || hit(in[i], B(i, r, t)[1]); p contributes iff
 *   it is not. Two draws of one peer are two messages.
 *   Ring mode (either list order): sender s, slot q in 0..2, target g =
 *   targets[3 s + q] is a message iff g exists and is alive; it is dropped iff
 *   hit(out[s], B(s, r, q)[0]) || hit(in[g], B(s, r, q)[1]).
 * Nothing else changes: the peer and placement draws are untouched, and with
 * loss off or both arrays all zero every table, statistic and diagnostic is
 * bit-identical.
 * gh_set_loss: out_q32 / in_q32 [N] by member id; one NULL pointer = that side
 * all zero; both NULL switch loss off and free its state. Every call zeroes
 * the counters. It takes effect from the next round run and persists across
 * gh_step, gh_import_state and gh_init_full (configuration, not table state).
 * gh_get_loss: *enabled, and the two arrays [N] (all 0 with loss off); any
 * output may be NULL. gh_loss_stats: *sent = the gossip messages and *dropped
 * = the dropped ones since the last gh_set_loss (either may be NULL);
 * GH_EINVAL with loss off. A NULL handle returns GH_EINVAL from all three
 * before any device is touched.
 * Off is the default: gh_create allocates nothing for it, gh_footprint and
 * gh_memory_info at creation do not include it, and gh_step launches nothing
 * new in either state (the kernels that build the inboxes take one uniform
 * branch). Enabled it holds 8 N + 16 bytes per shard (the arrays are
 * replicated). Additive under ABI 7. On a sharded handle all three calls are
 * collective: every rank passes the same arguments and gets the global
 * result. */
#define GH_LOSS_NEVER 0u
#define GH_LOSS_ALWAYS 0xFFFFFFFFu
int gh_set_loss(void* h, const uint32_t* out_q32, const uint32_t* in_q32);
int gh_get_loss(void* h, int32_t* enabled, uint32_t* out_q32, uint32_t* in_q32);
int gh_loss_stats(void* h, int64_t* sent, int64_t* dropped);

/* Network partitions (SPEC §2 step 6b): every member m is on side[m] in
 * [0, GH_PART_SIDES); reach(a, b) = side[a] == side[b]. Between members that
 * do not reach each other nothing is delivered: gossip, REMOVE, LEAVE and
 * JOIN. (gh_set_loss cannot express this: its REMOVEs, LEAVEs and JOINs stay
 * reliable, SPEC D9.)
 *   Gossip: a pull draw (receiver i, draw t, peer p) that is valid, or a ring
 *   message (sender s, slot q, target g existing and alive), is CUT iff the
 *   two do not reach each other. A cut message does not merge, adds 1 to the
 *   counter `cut`, and is no message for gh_set_loss: neither sent nor
 *   dropped, no LINK block drawn. The peer draws do not change.
 *   REMOVE: the recipients are fixed by the sides in force in the round of
 *   the detection. With n_j(c) = the detectors of c on row j's side and
 *   m_j(c) the lowest of them, row j applies REMOVE(c) in the next round iff
 *   it is alive, n_j(c) > 0 and not (n_j(c) == 1 and m_j(c) == j): rule D4 per
 *   side. det_cnt / det_min, gh_read_failed, gh_read_detectors, the stats and
 *   the journal stay global. A call between two rounds does not change who
 *   receives the REMOVE set already pending.
 *   Events, by the sides in force in the round that runs them: LEAVE(c)
 *   reaches j iff reach(c, j); a joiner's process starts fresh on any side;
 *   its JOIN reaches the introducer I iff reach(c, I); I's broadcast reaches j
 *   iff reach(I, j).
 *   Not gated: gh_merge_list, the file calls, gh_vote_scan, gh_rebuild_meta,
 *   gh_census, gh_file_audit.
 * After a heal, two sides that have dropped each other never re-merge by
 * gossip (a member only sends to members of its own list, and only lists it
 * is a member of reach it); they re-merge only through a JOIN.
 * gh_set_partition: side [N] by member id; a value outside [0, GH_PART_SIDES)
 * returns GH_EINVAL and changes nothing. NULL heals (every member to side 0);
 * the state stays allocated until gh_destroy. Every call zeroes `cut`. The
 * sides are configuration: they persist across gh_step, gh_import_state and
 * gh_init_full and take effect from the next round run. With all sides equal
 * every table, statistic, list and diagnostic equals a never-partitioned
 * engine's, and cut == 0.
 * NOT SUPPORTED, GH_EINVAL: a sharded handle (world > 1) and a GH_REMOVE_LIST
 * engine (both out of scope so far); never anywhere else.
 * gh_get_partition: *armed, and side [N] (all 0 when not armed); any output
 * may be NULL. gh_partition_stats: *cut since the last gh_set_partition;
 * GH_EINVAL when the engine is not armed. A NULL handle returns GH_EINVAL from
 * all three before any device is touched.
 * Before the first gh_set_partition nothing is allocated or launched
 * (gh_footprint and gh_memory_info at creation do not change; the inbox
 * kernels take one uniform branch on a null pointer). The first call ARMS the
 * engine: it allocates side[] and three bitmaps of ld * ceil(N / 32) words
 * (the recipients of two REMOVE sets and the detectors of a sweep; 3 x 512 MiB
 * at N = 65,536) and switches REMOVE delivery to per-(row, member) recipients
 * read from a bitmap, as a GH_REMOVE_LIST engine's. From then on a round with
 * a detection also builds the detectors' bitmaps and the recipients of D_r
 * (csrc/remove.hip k_part_recv). Additive under ABI 7.
 * Measured on a MI355X at N = 65,536, k = 4 pull (profiles/partition_time.json):
 * never armed 2.14 ms per round (the parent commit: 2.10-2.21 over three
 * processes); armed with every member on side 0, 2.18 ms; the two REMOVE
 * rounds of a 1 % crash 7.9 ms each (never armed 2.5 ms, a GH_REMOVE_LIST
 * engine 9.0 ms) and its detection rounds 5.2 ms (2.3 / 7.4 ms). A real split
 * is a heavier workload: with the members split even / odd the rounds stay at
 * 2.1 ms for 9 rounds and reach 17-36 ms by rounds 10-15. That jump was not
 * profiled; the supposed cause is the views that lag once half the draws are
 * cut, which the round kernels take off their fast path. */
#define GH_PART_SIDES 64
int gh_set_partition(void* h, const int32_t* side);
int gh_get_partition(void* h, int32_t* armed, int32_t* side);
int gh_partition_stats(void* h, int64_t* cut);

/* Lossy control messages (SPEC §2 step 6c, §5, D9): which of the control
 * messages cross the lossy links of gh_set_loss. `kinds` is a mask of
 * GH_CTL_REMOVE, GH_CTL_LEAVE and GH_CTL_JOIN (the JOIN to the introducer and
 * the introducer's broadcast); the default, 0, is none and is the engine before
 * this call existed. It acts only while gh_set_loss is on, with that call's
 * out[] / in[] thresholds and hit(). W(tag; a, r, b) = the Philox4x32-10 block
 * of counter (a, r, tag, b) under the engine's seed, r = the round being run;
 * word 0 is tested against the sender's out threshold, word 1 against the
 * receiver's in threshold. A message cut by a partition is no message: neither
 * counted nor drawn. Each decision is a pure function of its counter.
 *   REMOVE: det(c) = the rows that detected c in round r; E_j(c) = the
 *   detectors i != j with reach(i, j), whose Remove(c) messages row j. Message
 *   (i, j, c) draws Philox(K; i, j, 'CRMV' = 0x43524D56, 0) under the key K =
 *   words 0, 1 of W('CRMV'; c, r, 0), and is dropped iff hit(out[i], w0) ||
 *   hit(in[j], w1). Row j applies REMOVE(c) in round r + 1 iff it is alive
 *   then and some message of E_j(c) was not dropped. The thresholds, kinds and
 *   sides of round r decide; later calls do not change a pending set. det_cnt
 *   / det_min, gh_read_failed, gh_read_detectors, the stats and the journal
 *   stay global.
 *   LEAVE(c) to j (SPEC §5's conditions and reach(c, j)): dropped by
 *   W('LEAV' = 0x4C454156; c, r, j) against out[c], in[j].
 *   JOIN of c (c != I, I alive, reach(c, I)): dropped by W('JOIN' =
 *   0x4A4F494E; c, r, I) against out[c], in[I]; the joiner's process restarts
 *   whatever happens, and the introducer adds (and in append order appends)
 *   only the joiners it heard. Its broadcast to j: dropped by W('BCST' =
 *   0x42435354; I, r, j) against out[I], in[j]. A joiner c == I is local.
 * gh_set_control_loss: kinds outside 0..7 returns GH_EINVAL. Configuration: it
 * persists across gh_step, gh_import_state and gh_init_full and takes effect
 * from the next round run. With GH_CTL_REMOVE on an engine never armed it arms
 * the engine exactly as gh_set_partition(NULL) would (same allocations, every
 * member on side 0, a pending REMOVE set filled by rule D4); on an armed engine
 * sides and `cut` are left alone; without GH_CTL_REMOVE nothing is armed. With
 * loss off, or both threshold arrays all zero, every table, statistic, list and
 * diagnostic is bit-identical to kinds = 0. Every call zeroes the counters, and
 * so does gh_set_loss.
 * gh_control_loss_stats: out8 = remove_pairs (the (j, c) with E_j(c) non-empty
 * and j alive as round r ran), remove_missed (those with every message
 * dropped), leave_sent, leave_dropped, join_sent, join_dropped, bcast_sent,
 * bcast_dropped. REMOVE counts pairs, not messages: only "did any arrive" is
 * observable. GH_EINVAL until gh_set_control_loss has been called once.
 * NOT SUPPORTED, GH_EINVAL: a sharded handle (world > 1) and a GH_REMOVE_LIST
 * engine. A NULL handle returns GH_EINVAL from all three before any device is
 * touched. Before the first call nothing is allocated or launched (gh_footprint
 * and gh_memory_info do not change). Additive under ABI 7. */
#define GH_CTL_REMOVE 1
#define GH_CTL_LEAVE 2
#define GH_CTL_JOIN 4
int gh_set_control_loss(void* h, int32_t kinds);
int gh_get_control_loss(void* h, int32_t* kinds);
int gh_control_loss_stats(void* h, int64_t* out8);

/* MergeMemberList (slave/slave.go:414-440) of one received list into the
 * observer's row at the engine's current tick (the last completed round):
 * ids[x] (distinct members) with heartbeats hb[x] >= 0; the remote ts is
 * ignored (:426, :437). Present members advance when hb is larger, absent
 * ones are added, tombstoned ones are left alone. A stopped observer does
 * not receive (GetMsg runs while Alive). *merged = cells changed. Decoding
 * a reference datagram into (ids, hb) is the host's codec. */
int gh_merge_list(void* h, int32_t observer, const int32_t* ids, const int32_t* hb, int64_t n,
                  int64_t* merged);

/* "put" placement: Handle_put_request (master/master.go:152) for n distinct
 * files. replicas: [n][replicas] (-1 padded), versions [n], status [n]
 * (GH_OK / GH_EPLACEMENT_STARVED). Returns GH_EPLACEMENT_STARVED if any file
 * starved. */
int gh_put(void* h, const int32_t* files, int64_t n, int32_t* replicas,
           int32_t* versions, int32_t* status);
/* If_file_updated_recent (master/master.go:214-229) for n files: conflict[x]
 * = 1 if the file exists and was put less than `window` rounds ago (the
 * reference's 60 s write-write window at 1 s rounds: window = 60). The put
 * path asks for confirmation on a conflict (server/server.go:79-114). */
int gh_put_conflicts(void* h, const int32_t* files, int64_t n, int32_t window, uint8_t* conflict);
/* Update_metadata (master/master.go:74) with available = observer's list;
 * plan entries in file order. *n_plan = number of entries (<= cap written).
 * Every file's metadata is repaired. GH_DETECT_QUIRK engines also keep the
 * reference's plan-map remake (:118, SPEC D5): the plan holds only the entry
 * of the highest repaired file id (Go's map order is random, so which file
 * the reference returns is unpinned). */
int gh_repair(void* h, int32_t observer, gh_plan_entry* plan, int64_t cap,
              int64_t* n_plan);
/* get / ls (master/master.go:177-212): versions -1 if absent. */
int gh_get_files(void* h, const int32_t* files, int64_t n, int32_t* replicas,
                 int32_t* versions);
/* delete (master/master.go:249-259): old replicas returned. */
int gh_delete_files(void* h, const int32_t* files, int64_t n,
                    int32_t* old_replicas);

/* File-table audit: the master's replica table summarised against an
 * availability set, reduced on the device in one read-only pass over the file
 * slots (no reference counterpart: the reference learns this only by running
 * Update_metadata, master/master.go:74-127, which mutates the table). Defined
 * on the current file table and membership table; queued events are not
 * applied, and the table and the draw counters are unchanged.
 *   A (availability): observer in [0, N): the present members of that row
 *     (hb[observer][a] >= 0), exactly the `available` of Update_metadata
 *     (master/master.go:93-99), the set gh_repair(observer) uses. observer ==
 *     GH_AVAIL_ALIVE: the members with alive[a] as gh_export_state returns it
 *     now, the ground truth no member of the reference can see. Any other
 *     value: GH_EINVAL.
 *   A file f exists iff its version is >= 0. Its working count w(f) = the
 *     replica slots q < R with 0 <= rep[f][q] < N and rep[f][q] in A: slots,
 *     not distinct members, as Update_metadata appends them (:93-99).
 *   *files = the existing files.
 *   working_hist[b], b < GH_AUDIT_BINS = the existing files with w(f) == b
 *     (bins above R are 0). working_hist[0]: no working replica (alive mode:
 *     the file is lost). The sum over b < R is the number of entries
 *     gh_repair(observer) would plan (in GH_DETECT_CANONICAL its *n_plan).
 *   *starved = of the files with w < R, those Init_replica would refuse for
 *     one of its two preconditions (master/master.go:129-135), with the
 *     current master's candidate list as gh_put / gh_repair obtain it (list
 *     order under GH_ORDER_APPEND), M its length: M <= 1 (Intn panics), or
 *     (M - 1) - in_pool < R - w, in_pool = the working slots naming a
 *     candidate other than the last (the last is never drawn, :135; the loop
 *     would not end). The 2^20-draw budget of one placement is not predicted.
 *   load[m] = the existing files with at least one slot naming m (a member
 *     named twice by one file counts once): len(store(m)), the `store`
 *     command (slave/slave.go:605, sdfs_slave/sdfs_slave.go:59-68) read from
 *     the master's metadata. Independent of A.
 *   sole[m] = the existing files with w(f) == 1 whose one working slot names
 *     m: the files that die with m.
 * working_hist: [GH_AUDIT_BINS]; load, sole: [N] by member id; any output may
 * be NULL. Additive under ABI 7. On a sharded handle both calls are
 * collective: every rank calls them with the same arguments (the same outputs
 * NULL), and every rank gets the global result. GH_EINVAL for an engine
 * created with max_files = 0. */
#define GH_AVAIL_ALIVE (-1)   /* availability = the running processes      */
#define GH_AUDIT_BINS 9       /* working replicas 0..8 (replicas is 1..8)  */
int gh_file_audit(void* h, int32_t observer, int64_t* files, int64_t* working_hist,
                  int64_t* starved, int32_t* load, int32_t* sole);
/* The existing files f, in ascending id, with (member < 0 or some slot of f
 * names `member`) and w(f) <= max_working under the A of `observer` (as
 * above); max_working in 0..8, max_working >= R disables the condition.
 * *n_out = their number, the lowest min(*n_out, cap) ids are written.
 * (any observer, m, 8) is the `store` command at m (slave/slave.go:605);
 * (GH_AVAIL_ALIVE, -1, 0) the lost files; (o, -1, R - 1) the files
 * gh_repair(o) would touch; (GH_AVAIL_ALIVE, m, 1) the files lost if m
 * died. GH_EINVAL for member >= N, max_working outside 0..8, a bad observer,
 * or a NULL n_out / NULL files with cap > 0. */
int gh_file_select(void* h, int32_t observer, int32_t member, int32_t max_working,
                   int32_t* files, int64_t cap, int64_t* n_out);

/* ---- master re-election (SPEC §9; slave/slave.go:930-1051) ------------- */
/* The master check at the end of updateMemberList (slave/slave.go:451-457)
 * and revote_master's target (:930-948), for every row of the current table:
 * list_len[i] = len(MemberList_i); has_master[i] = 1 if member mview[i] (row
 * i's own idea of the master, self.master) is in row i's list; first[i] =
 * MemberList_i[0] (under GH_ORDER_ID the lowest present member id, SPEC D1),
 * -1 for an empty list. mview: [N] member ids. Outputs: [N] each; any output may be NULL.
 * The vote tally (Receive_vote :968-984, RPC TCPServer.Vote
 * server/server.go:231) is per-candidate control flow and stays on the host
 * (gossipsim.Cluster). */
int gh_vote_scan(void* h, const int32_t* mview, int32_t* first, int32_t* list_len,
                 uint8_t* has_master);
/* rebuild_file_meta (slave/slave.go:986-1043) run by the newly elected
 * master M: the file table is rebuilt from the members' local stores as the
 * reference reads them (M's own, and MemberList_M[0]'s for every other member,
 * :994), Node_list = the first 4 entries in ascending-version order, Version
 * = the first entry's, Timestamp = the current tick; files in no store read
 * are dropped. M becomes the engine's master row (placement candidates,
 * gh_put/gh_repair). *f0 = MemberList_M[0] (the member that receives
 * Assign_new_master, :1000 / server/server.go:236), may be NULL;
 * *n_files = files left in the table, may be NULL. GH_EINVAL if M's list is
 * empty. */
int gh_rebuild_meta(void* h, int32_t new_master, int32_t* f0, int64_t* n_files);
/* A master's file metadata (its SDFSMaster maps, master/master.go:38-44) as
 * flat arrays over files 0..max_files-1: replica lists [F][R] (-1 = none),
 * versions [F] (-1 = no such file), put timestamps [F], placement draw
 * counters [F]. gh_export_files copies the engine's table out (every rank gets
 * the whole table); gh_import_files replaces it (every rank takes its own
 * files). A master demoted by an election while its process kept running
 * (slave/slave.go:1122-1175: members whose self.master still names it send
 * their Update_metadata calls there) answers from its own maps: a host keeps
 * them beside the engine's and swaps them in, with gh_set_master, to run
 * those calls (gossipsim.Cluster). */
int gh_export_files(void* h, int32_t* replicas, int32_t* versions, int32_t* timestamps, uint32_t* draws);
int gh_import_files(void* h, const int32_t* replicas, const int32_t* versions, const int32_t* timestamps,
                    const uint32_t* draws);
/* The member whose list is the master's Member_list (placement candidates of
 * gh_put / gh_repair, master/master.go:46); gh_create takes gh_config.master,
 * gh_rebuild_meta sets the new master. */
int gh_set_master(void* h, int32_t master);

/* ---- multi-GPU: one cluster column-sharded over G ranks ----------------
 * Rank g holds all N observer rows for member columns [g*ncs, g*ncs+ncol)
 * (ncs = roundup(ceil(N/G), 32)): 4*N*ncs bytes of narrow table plus arenas.
 * Merge, detection, cleanup and REMOVE delivery of a member happen on its
 * column's rank; per round the ranks exchange only O(N) vectors (present
 * counts, pull inboxes or ring positions/targets) by RCCL over xGMI. This
 * replaces the reference's per-host processes exchanging UDP lists
 * (slave/slave.go:499-544) for a simulated cluster spread over GPUs.
 * SPMD contract: every rank calls every gh_* function of a sharded handle
 * with the same arguments in the same order (most calls are collective);
 * every rank returns the same (global) results. */
#define GH_COMM_RCCL 0    /* one process per GPU, RCCL over xGMI              */
#define GH_COMM_LOCAL 1   /* ranks are threads of one process (any devices)  */
#define GH_COMM_ID_BYTES 128
/* Shard layouts (DESIGN.md "Multi-GPU"):
 *   GH_LAYOUT_COLUMNS  rank g holds member columns [g*ncs, g*ncs + ncs) of
 *                      ALL rows; every per-round exchange is O(N) (default)
 *   GH_LAYOUT_ROWS     rank g holds observer rows [g*nrs, g*nrs + nrs) with
 *                      ALL columns (north_star): each round the senders'
 *                      rows that a shard's receivers pull cross shards by
 *                      one alltoallv (ncclAllToAllv), O(N^2 k/G) bytes.
 *                      Pull and ring mode: in ring mode each sender's owner
 *                      finds its 3 targets in its own row, the targets are
 *                      reduced, and the senders' rows travel to their
 *                      receivers' owners the same way. */
#define GH_LAYOUT_COLUMNS 0
#define GH_LAYOUT_ROWS 1

/* RCCL unique id for gh_create_sharded (call on rank 0, send to all). */
int gh_comm_unique_id(uint8_t* id);
/* comm_id: GH_COMM_RCCL -> the unique id; GH_COMM_LOCAL -> a NUL-terminated
 * group key shared by the ranks (<= GH_COMM_ID_BYTES). world == 1 needs no
 * transport (comm_id may be NULL). cfg->device selects the rank's GPU. */
int gh_create_sharded(const gh_config* cfg, int32_t rank, int32_t world, int32_t transport,
                      const uint8_t* comm_id, void** handle);
int gh_shard_info(void* h, int32_t* rank, int32_t* world, int64_t* col0, int64_t* ncols);

/* Table encoding of this engine's shard (diagnostic; DESIGN.md "Data layout"):
 * (tile, row) segments of the current table held wide (arena or frozen
 * store, stopped rows included); segments the last round ran through the per-cell
 * rule (k_round_slow); the round kernel variant of the last round (0 lean,
 * 1 storm) and its storm measure; the row segments the last round skipped as
 * quiet (inactive rows that stopped changing). Any output may be NULL. No
 * reference counterpart. */
int gh_encoding_info(void* h, int64_t* wide_segments, int64_t* slow_segments, int32_t* storm_mode,
                     int64_t* storm_segments, int64_t* quiet_segments);
/* Sender snapshot plane (diagnostic; DESIGN.md "Sender plane"): whether the
 * engine keeps one (pull mode, 3 <= k <= 4, N >= 16,384), whether the current table's plane is
 * valid for the next round, and how many waves of the last round gathered
 * 16-bit sender codes although the plane was valid (a sender code outside
 * the plane's window). Any output may be NULL. No reference counterpart. */
int gh_plane_info(void* h, int32_t* enabled, int32_t* valid, int64_t* fallback_waves);
/* 4-bit tier (diagnostic; DESIGN.md "4-bit tier"): whether the engine keeps
 * one (plane mode, column layout; GH_C8=0 drops it), whether the current
 * table is held in it (lag and age nibbles, escaped chunks in 16 bits), how
 * many chunks the last round's packed 16-bit path wrote escaped, and the
 * round kernel variant of the last round (0 lean on a 16-bit input, 1 storm,
 * 2 lean on a tier input widened to 16 bits, 3 the nibble path). Any output
 * may be NULL. No reference counterpart. */
int gh_tier_info(void* h, int32_t* enabled, int32_t* current_8bit, int64_t* escaped_chunks, int32_t* last_variant);
/* Lane jobs of the nibble path (diagnostic; DESIGN.md "Lane jobs"): in the
 * last round, the lanes (16 cells of a row) whose cells left the 4-bit tier
 * or needed the per-cell rule -- crashed members' aging, flagged and
 * tombstoned cells, REMOVE -- and were done by k_round_jobs instead of
 * sending their whole 256-cell segments to the slow list, and how many of
 * them needed a wide segment (k_round_redo). Any output may be NULL. No
 * reference counterpart. (ABI 6) */
int gh_job_info(void* h, int64_t* lane_jobs, int64_t* redo_lanes);
/* Row layout (GH_LAYOUT_ROWS): the last ghost-row exchange of this shard --
 * the sender rows it received, and the bytes it sent and received by
 * alltoallv (narrow codes, plane words, wide segments). Zero in the column
 * layout, whose exchanges are O(N) collectives. Any output may be NULL. No
 * reference counterpart (it replaces the UDP list pushes, slave/slave.go:527-542). */
int gh_exchange_info(void* h, int64_t* ghost_rows, int64_t* bytes_out, int64_t* bytes_in);
/* HBM held by the tables (narrow x2 + wide arenas + frozen store), wide-arena
 * slots in use / per buffer, and stopped rows in the frozen store. Any
 * output may be NULL. Diagnostic; no reference counterpart. */
int gh_memory_info(void* h, int64_t* device_bytes, int64_t* wide_used, int64_t* wide_cap, int64_t* frozen_rows);
/* The file table of this engine / shard (placement is per file,
 * master/master.go:74-150): sharded by file ID, file f on shard f % G at slot
 * f / G, so *slots = ceil(max_files / G) files' replica lists, versions and
 * timestamps; *shards = G (1 for one engine); *held = the files put and not
 * deleted in this shard's slots. Any output may be NULL. Diagnostic. */
int gh_file_info(void* h, int64_t* slots, int32_t* shards, int64_t* held);
/* The A/B and diagnostic switches this engine runs with (diagnostic; read-only).
 * gh_create reads each from the environment variable GH_<name> once, so an
 * engine keeps the values of its creation and the next engine of the process
 * may get others; results never depend on them (DESIGN.md measures against
 * each). out[GH_KNOB_x] = the value in effect: QUIRK_ROWS 1 the one-pass
 * quirk pre-pass where it applies (0 the two-sweep one); JOBS_FLAT 1 lane
 * jobs dealt one per lane (0 by region); RMV_FULL7 1 the full-grid REMOVE
 * launch without a block loop; DNW / NREC 1 the nibble path's move words /
 * row records are kept (0 also where they do not apply: shards);
 * FORCE_SLOW / FORCE_STORM every segment by the
 * per-cell rule / the storm variant every round; ROUND_NT, ROUND_TPW,
 * ROUND_XMAP k_round's non-temporal streams, tiles per workgroup and tile
 * map; SLOW_GRID workgroups of the per-cell kernel; NIB_RMV REMOVE
 * on the nibble path; GX_DIRECT same-device row shards
 * gather their ghosts' planes in place; TMODE the timing mode; PLANE, C8 the
 * sender plane and the 4-bit tier are kept; TILE_W the members per table tile
 * this engine (or shard) runs with: gh_config.tile_width, or its default with
 * and without the sender plane, or GH_TILE_W where that is set. Writes
 * min(n_out, GH_KNOB_COUNT) values; *count (may be NULL) = GH_KNOB_COUNT. No
 * reference counterpart. */
enum {
  GH_KNOB_QUIRK_ROWS = 0, GH_KNOB_JOBS_FLAT, GH_KNOB_RMV_FULL7, GH_KNOB_DNW, GH_KNOB_NREC, GH_KNOB_FORCE_SLOW,
  GH_KNOB_FORCE_STORM, GH_KNOB_ROUND_NT, GH_KNOB_ROUND_TPW, GH_KNOB_SLOW_GRID, GH_KNOB_NIB_RMV, GH_KNOB_GX_DIRECT,
  GH_KNOB_ROUND_XMAP, GH_KNOB_TMODE, GH_KNOB_PLANE, GH_KNOB_C8, GH_KNOB_TILE_W, GH_KNOB_COUNT
};
int gh_debug_knobs(void* h, int32_t* out, int64_t n_out, int64_t* count);
/* The HBM one shard (rank of world, layout and sizes from cfg) would hold,
 * without a device or a communicator (a dry walk of gh_create's
 * allocations): *create_bytes = everything gh_create allocates;
 * *exchange_bytes = the row layout's ghost-row exchange buffers at a
 * healthy pull round's expected distinct remote senders (0 in the column
 * layout). The frozen store (grows with stopped rows) and per-call staging
 * are not included. Plans config 4 (N = 262,144 over 8 GPUs) before any
 * allocation. Any output may be NULL. No reference counterpart. */
int gh_footprint(const gh_config* cfg, int32_t rank, int32_t world, int32_t transport, int64_t* create_bytes,
                 int64_t* exchange_bytes);

/* Tuning knobs of the round kernel (k_round): non-temporal stores of the new
 * table and the XCD-aware block->tile map. Results do not depend on them;
 * the defaults (both on) are the measured fastest. */
int gh_set_round_variant(void* h, int32_t nontemporal, int32_t xcd_map);

/* Device timing of the fused round kernel (HIP events on the engine's
 * stream), for bench.py's roofline: enable, then read the sum of kernel
 * durations (ms) and launch count since enabling. */
int gh_set_timing(void* h, int32_t enable);
int gh_read_timing(void* h, double* total_ms, int64_t* launches);
/* Block until all queued device work has finished. */
int gh_sync(void* h);

/* Cluster ensembles (SPEC.md §11): B independent clusters of the same N
 * (2..GH_ENS_MAX_MEMBERS) and fanout behind one handle, each with its own
 * seed, T_fail, T_cleanup, per-member loss thresholds and round counter, all
 * advanced by one launch per gh_ens_step call: one workgroup owns one cluster
 * and runs every round of the call out of registers and LDS (DESIGN.md
 * "Ensemble"). For sweeps over seeds x loss rates x timeouts of small
 * clusters, where an engine's round is launch overhead. No reference
 * counterpart: the nearest is running the reference cluster (main.go:27-33,
 * about ten processes) B times.
 * Every cluster advances by SPEC §2 restricted to: the ensemble's peer_mode
 * (GH_PEER_PULL, the default, or GH_PEER_RING) and detect_mode
 * (GH_DETECT_CANONICAL, the default, or GH_DETECT_QUIRK), GH_ORDER_ID,
 * GH_REMOVE_ALL (D4), GH_EV_CRASH events, the lossy links of step 6a. The two
 * modes are per ensemble, not per cluster; a config with both words 0 is the
 * ensemble of before they existed. Cluster b is bit for bit what a gh_create
 * engine with the same peer_mode and detect_mode, params[b]'s seed and
 * timeouts, the same N, fanout and min_members, the same crashes and
 * gh_set_loss(out[b], in[b]) computes: tables, alive, every gh_round_stats
 * field (ring_empty included), the failed set, sent / dropped.
 *   GH_PEER_RING (slave/slave.go:512-524, SPEC §2 step 6 "Ring mode", the
 *   list in member-ID order): every running active sender s takes the present
 *   cells of its row after steps 1-5, L of them, idx = the rank of s among
 *   them or -1; its three targets are list[(idx-1) mod L], list[(idx+1) mod L],
 *   list[(idx+2) mod L] (Go's truncated % plus L for negatives); L = 0 counts
 *   one ring_empty and sends nothing. Slot q in {0,1,2} to a running target g
 *   is a message (sent), dropped iff hit(out[b][s], B(s, r, q)[0]) ||
 *   hit(in[b][g], B(s, r, q)[1]) under the cluster's seed. With L < 4 a sender
 *   may target one member twice, or itself: each slot is its own message,
 *   and the merge takes the max over the distinct arrived senders. fanout is
 *   validated (1..8) and otherwise unused, as on an engine.
 *   GH_DETECT_QUIRK (slave/slave.go:464-477, SPEC §4, on the ID-ordered
 *   list of an active row i after steps 1-3): c is a candidate iff c != i,
 *   hb > 1, ts < r - T_fail; within each run of consecutive candidates the
 *   ones at even offsets are detected, and the list's last entry always; a
 *   skipped candidate stays present with its stale ts and is met again next
 *   round.
 * Not supported (use an engine): append order, GH_REMOVE_LIST, joins and
 * leaves, partitions, lossy control messages, files, election, shards,
 * N > 128.
 *   State: per cluster SPEC §1's tables, alive and round, plus the pending
 *   REMOVE set D_{r-1} (per member the rows that detected it and the lowest
 *   of them). It persists between gh_ens_step calls: R calls of one round
 *   equal one call of R rounds. gh_ens_create leaves every cluster empty (no
 *   cell, nobody running, round 0). gh_ens_init_full: every cluster, every
 *   row alive holding every member at (hb0, ts0) (hb0 < 0: GH_ERANGE).
 *   gh_ens_import_state: one cluster's hb [N][N], ts [N][N], alive [N] as
 *   gh_import_state takes them (hb < -2: GH_ERANGE, nothing imported). Both
 *   set the round counter (>= 0) and clear the cluster's pending REMOVE set
 *   and detect record; loss and queued events stay. gh_ens_export_state:
 *   clusters [cluster0, cluster0 + n) as hb / ts [n][N][N], alive [n][N],
 *   round [n], any of them NULL, with gh_export_state's two presentation
 *   rules (an absent cell's ts is 0; with T_cleanup < 30 a tombstone older
 *   than T_cleanup + 1 rounds exports ts = round + 1 - (T_cleanup + 1)).
 *   Events: gh_ens_apply_events queues GH_EV_CRASH of the listed members for
 *   the next round run (step 0), in one cluster or with cluster = -1 in every
 *   cluster. Any GH_EV_JOIN / GH_EV_LEAVE (or unknown kind) in the list:
 *   GH_EINVAL, and nothing of the list is queued.
 *   Rounds: gh_ens_step runs `rounds` >= 0 rounds of every cluster, steps 0-6a
 *   in SPEC order: events; REMOVE delivery to every running row but a sole
 *   detector; the <min_members guard (a guarded row stamps ts = r on its
 *   listed members, skips steps 3-5, still receives); own heartbeat; detect
 *   (c != i, hb > 1, ts < r - T_fail; the quirk sweep skips some); clean
 *   (ts < r - T_cleanup); in pull mode the merge from the snapshot of the k
 *   peers Philox(seed; i, r, 'PEER', t / 4)[t % 4] -> other_i, in ring mode
 *   from the senders that targeted the row. stats (may be NULL) [B]: s = exactly an engine's
 *   gh_round_stats summed over the call (ring_empty is 0 in pull mode); false_failed = sum
 *   over rounds of the running members detected, false_detections = those
 *   members' detecting cells (gh_journal_round's fields, summed); sent /
 *   dropped = step 6a's counters over this call.
 *   Loss: gh_ens_set_loss takes out_q32 / in_q32 [B][N] (NULL = that side all
 *   zero); hit(), B(a, r, blk) and the pull-mode and ring-mode rules are
 *   gh_set_loss's, under the cluster's own seed. sent / dropped are always counted; with every
 *   threshold zero each table and statistic equals the lossless run. Loss is
 *   configuration: it persists across import and gh_ens_init_full.
 *   gh_ens_read_failed: the last round's D_r per cluster as bitmaps
 *   [B][ceil(N / 32)] (all zero after an import). gh_ens_read_detect, [B][N]
 *   each, either NULL: first_round[b][c] = the first round since the last
 *   import / gh_ens_init_full of cluster b in which c was detected while not
 *   running (-1: never); fp_rounds[b][c] = the rounds in which c was detected
 *   while running (the journal's definitions).
 * Errors: GH_EINVAL, before any device is touched, for a NULL handle, cfg or
 * params, N outside 2..128, B < 1, fanout outside 1..8, a peer_mode or
 * detect_mode other than the two values each has, a negative
 * min_members / t_fail / t_cleanup / rounds / round, a cluster or member id
 * out of range. gh_ens_step returns GH_ERANGE and runs nothing when for some
 * cluster (the largest imported or initial hb) + (rounds run since) + rounds,
 * or its round counter + rounds, would pass INT32_MAX. GH_ENODEV without a
 * gfx950 device: as everywhere, no CPU fallback. A failed gh_ens_create leaves
 * *h NULL.
 * HBM: 8 B N^2 bytes of tables + 26 B N + 132 B bytes. A handle owns its own
 * buffers and stream; nothing is allocated, launched or changed for ordinary
 * engines. Additive under ABI 7. */
#define GH_ENS_MAX_MEMBERS 128
typedef struct gh_ens_config {
  int32_t n_members;     /* N, 2..GH_ENS_MAX_MEMBERS, the same for every cluster */
  int32_t n_clusters;    /* B >= 1                                           */
  int32_t fanout;        /* k, 1..8                                          */
  int32_t min_members;   /* the <4 guard (slave/slave.go:504), >= 0          */
  int32_t device;        /* HIP device ordinal                               */
  int32_t peer_mode;     /* GH_PEER_PULL (0, default) | GH_PEER_RING         */
  int32_t detect_mode;   /* GH_DETECT_CANONICAL (0, default) | GH_DETECT_QUIRK */
  int32_t reserved[1];
} gh_ens_config;
typedef struct gh_ens_params {   /* per cluster, 16 bytes */
  uint64_t seed;         /* Philox key of the cluster's peer and link draws  */
  int32_t t_fail;        /* PERIOD in rounds, >= 0                           */
  int32_t t_cleanup;     /* COOLDOWN in rounds, >= 0                         */
} gh_ens_params;
typedef struct gh_ens_stats {    /* per cluster, 14 x int64 */
  gh_round_stats s;         /* exactly an engine's, summed over the call     */
  int64_t false_failed;     /* Σ_rounds running members detected that round  */
  int64_t false_detections; /* those members' detecting cells                */
  int64_t sent;             /* gossip messages of this call (step 6a)        */
  int64_t dropped;          /* the dropped ones                              */
} gh_ens_stats;
int gh_ens_create(const gh_ens_config* cfg, const gh_ens_params* params, void** h);
void gh_ens_destroy(void* h);
const char* gh_ens_last_error(void* h);
int gh_ens_init_full(void* h, int32_t hb0, int32_t ts0, int32_t round);
int gh_ens_import_state(void* h, int64_t cluster, const int32_t* hb, const int32_t* ts,
                        const uint8_t* alive, int32_t round);
int gh_ens_export_state(void* h, int64_t cluster0, int64_t n, int32_t* hb, int32_t* ts,
                        uint8_t* alive, int32_t* round);
int gh_ens_set_loss(void* h, const uint32_t* out_q32, const uint32_t* in_q32);
int gh_ens_apply_events(void* h, int64_t cluster, const gh_event* ev, int64_t n);
int gh_ens_step(void* h, int32_t rounds, gh_ens_stats* stats);
int gh_ens_read_failed(void* h, uint32_t* bitmap);
int gh_ens_read_detect(void* h, int32_t* first_round, int32_t* fp_rounds);

#ifdef __cplusplus
}
#endif

#endif /* GOSSIPHIP_H_ */
