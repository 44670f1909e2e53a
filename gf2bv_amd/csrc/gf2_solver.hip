// gf2_solver.hip -- host side of libgf2bv_hip.so: the C ABI declared in include/gf2bv_hip.h.
//
// This is what gf2bv/_internal.c:398-489 (assembly -> _mzd_pluq -> _mzd_pluq_solve_left ->
// _mzd_kernel_left_pluq -> transpose) becomes on an MI355X: one uninterrupted stream of HIP
// launches per system; every data-dependent quantity (rank so far, pivots of the current
// panel, row moves) stays in device memory, so the host never synchronises mid-elimination.
//
// There is deliberately NO CPU fallback: without a HIP device every solve entry point
// returns GF2BV_ERR_NODEVICE.
#include "gf2_kernels.hip.h"
#include <hip/hip_ext.h>
#include "../../include/gf2bv_hip.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

thread_local std::string g_err = "";

int fail(int code, const char *what, hipError_t e = hipSuccess)
{
	char buf[512];
	if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
	else snprintf(buf, sizeof buf, "%s", what);
	g_err = buf;
	return code;
}

// Nothing may propagate through the C ABI: allocation failures of the host-side containers become GF2BV_ERR_NOMEM.
// GF2BV_RETRY_EVENTS (internal, never returned through the C ABI): a stream hand-over gate gave up on the device -- kernels
// of the two streams were not executing concurrently after all (a profiler attached since the probe, say).  The device
// has been marked accordingly (streams_run_concurrently) and the solve is repeated once, with the event hand-over: the
// input is never modified.
#define GF2BV_RETRY_EVENTS (-77)
thread_local int g_attempt = 0;      // attempt of the running C-ABI call (gf2bv_stats::handover_retries)
template <class F>
int catching(F &&body)
{
	try { return body(); }
	catch (const std::bad_alloc &) { return fail(GF2BV_ERR_NOMEM, "out of host memory"); }
	catch (const std::exception &e) { return fail(GF2BV_ERR_HIP, e.what()); }
}
template <class F>
int guarded(F &&body)
{
	for (int attempt = 0;; attempt++) {
		g_attempt = attempt;
		const int rc = catching(body);
		if (rc != GF2BV_RETRY_EVENTS) return rc;
		if (attempt) return fail(GF2BV_ERR_HIP, "a stream hand-over gate timed out on the device");
	}
}

#define HIPCHK(call)                                                     \
	do {                                                                 \
		hipError_t _e = (call);                                          \
		if (_e != hipSuccess) return fail(GF2BV_ERR_HIP, #call, _e);     \
	} while (0)

inline i64 round_up(i64 v, i64 m) { return (v + m - 1) / m * m; }
// k_update16k does not clamp its row indices: a tile's last chunk (an item: up to GF2_WSEG x 1024 rows) may read that far past the tile
// (never stored); the working matrix and the multiplier sets get this much slack behind them
constexpr size_t kOuterSlackBytes = (size_t)GF2_WSEG * 1024 * 32;   // (the largest item of the outer pass's workgroup shapes: 12288 rows)

// ---- environment switches -----------------------------------------------------------------------
// Every GF2BV_* variable this library reads, described where read() -- the only function of this file that reads the environment --
// parses it (the members' initialisers are the defaults; DESIGN.md section 8 adds lifetimes, users and history).  Members hold what was
// ASKED for: what a solve makes of it is Solver state.  flag: on iff set, whatever the text; value: set, "" included (atoi("") is 0);
// non-empty: "" counts as unset; tri-state: a value, -1 while unset.  Read at every entry that needs it; slab_pad and keep_big are latched.
struct Knobs {
	bool plain = false, outer_chain = false, serial = false, ysweep = false, small_probe = false, trace = false, two_level_min_set = false;
	bool outer_side = true, fast = true, fused_narrow = true, sparse_fast = true, pc = true, gang_nt = true, gang_bs = true, small = true, keep_big = true;
	int stream_pairs = -1, two_level = -1, optimistic = -1, xcd_pin = -1, bs_inv = -1, small_zc = -1;          // tri-states (two_level: -1 by size, 0 off, else K)
	int update = 0, flag_sync = 1, xcd_wgs = 32, self_wait_us = 50, gang = 0, batch_threads = 2, debug_sync = 0;
	i64 slab_pad = 64, host_pool_mb = 4608;
	double two_level_min_mib = 512;
	static constexpr int kNumUpdates = 6;
	enum Part { kAll, kSmall, kHostPool };      // what an entry reads: the small path and gf2bv_host_free only their own (the lookups they always made)
	static Knobs read(Part what = kAll)
	{
		Knobs k;
		if (const char *e = getenv("GF2BV_HOST_POOL_MB")) { const long v = atol(e); if (v >= 0) k.host_pool_mb = v; }      // value, >= 0 (else 4608): MiB of idle page-locked staging gf2bv_host_free keeps
		if (what == kHostPool) return k;
		if (const char *e = getenv("GF2BV_SMALL")) k.small = atoi(e) != 0;      // value, on: 0 sends small systems down the blocked path
		if (const char *e = getenv("GF2BV_SMALL_ZC")) k.small_zc = atoi(e) != 0;      // tri-state (unset: up to 32 KiB): the small path reads its input over the link, never / always
		k.small_probe = getenv("GF2BV_SMALL_PROBE") != nullptr;      // flag: the small path's phase times on stderr
		if (what == kSmall) return k;
		if (const char *e = getenv("GF2BV_PLAIN")) k.plain = atoi(e) != 0;      // value: != 0 turns stream pairing, XCD pinning, flag hand-overs and the optimistic enqueue off by default
		if (const char *e = getenv("GF2BV_STREAM_PAIRS")) k.stream_pairs = atoi(e) != 0;      // tri-state (unset: !plain): 0 gives a single solve any idle bulk stream, not a probed one
		if (const char *e = getenv("GF2BV_UPDATE")) { const int v = atoi(e); if (v >= 0 && v < kNumUpdates) k.update = v; }      // value: index into kUpdates, anything outside it is 0
		if (const char *e = getenv("GF2BV_TWO_LEVEL"); e && *e) { const int v = atoi(e); k.two_level = v <= 0 ? 0 : std::min(GF2_KMAX, std::max(2, v)); }      // non-empty: <= 0 is 0, no outer panels; else K = clamp(v, 2, GF2_KMAX) forced; unset: by size
		if (const char *e = getenv("GF2BV_TWO_LEVEL_MIN_MIB"); e && *e) { k.two_level_min_set = true; k.two_level_min_mib = atof(e); }      // non-empty (unset: 512, or 0 under a forced K): outer panels while more than this many MiB remain right of them
		if (const char *e = getenv("GF2BV_OUTER_CHAIN"); e && *e) k.outer_chain = atoi(e) != 0;      // non-empty, off: != 0 runs the chain of panel steps on every word group instead of P = T x S
		if (const char *e = getenv("GF2BV_OUTER_SIDE"); e && *e) k.outer_side = atoi(e) != 0;      // non-empty, on: 0 puts the outer step on the next panel's tiles in front of the pass, not beside it
		if (const char *e = getenv("GF2BV_FAST")) k.fast = atoi(e) != 0;      // value, on: 0 never tries the one-launch block search
		if (const char *e = getenv("GF2BV_OPTIMISTIC")) k.optimistic = atoi(e) != 0;      // tri-state (unset: !plain): 0 enqueues the general panel steps behind every search
		if (const char *e = getenv("GF2BV_FUSED_NARROW")) k.fused_narrow = atoi(e) != 0;      // value, on: 0 runs search and narrow step of an optimistic block as two launches
		if (const char *e = getenv("GF2BV_SPARSE_FAST")) k.sparse_fast = atoi(e) != 0;      // value, on: 0 sends sparse systems through the general panel steps
		if (const char *e = getenv("GF2BV_PC")) k.pc = atoi(e) != 0;      // value, on: 0 lets the bulk update fetch the pivot rows through the panel records
		if (const char *e = getenv("GF2BV_FLAG_SYNC")) k.flag_sync = atoi(e);      // value, 1: 0 hands over through events; 2 skips the concurrency probe (the expired-gate path)
		k.serial = getenv("GF2BV_SERIAL") != nullptr;      // flag: panel and bulk path on ONE stream
		if (const char *e = getenv("GF2BV_XCD_PIN")) k.xcd_pin = atoi(e) != 0;      // tri-state (unset: off under plain, else the dispatch probe): a gang's systems each on one XCD
		if (const char *e = getenv("GF2BV_XCD_WGS")) k.xcd_wgs = std::min(256, std::max(1, atoi(e)));      // value, clamp(v, 1, 256): bulk-update workgroups per system of a pinned gang
		if (const char *e = getenv("GF2BV_GANG_NT")) k.gang_nt = atoi(e) != 0;      // value, on: 0 gives pinned gangs plain instead of streaming row accesses
		if (const char *e = getenv("GF2BV_GANG_BS")) k.gang_bs = atoi(e) != 0;      // value, on: 0 runs one back-substitution chain per system of a gang
		if (const char *e = getenv("GF2BV_BS_INV")) k.bs_inv = atoi(e) != 0;      // tri-state (unset: from 16 panel groups up): diagonal blocks inverted up front, never / always
		k.ysweep = getenv("GF2BV_YSWEEP") != nullptr;      // flag: every back-substitution through the table sweeps over Y
		if (const char *e = getenv("GF2BV_SELF_WAIT_US")) { const int v = atoi(e); if (v >= 0 && v <= 1000000) k.self_wait_us = v; }      // value, 0 .. 1000000 (else 50): a search's unit 0 hands publishing over after this long; 0 never waits
		if (const char *e = getenv("GF2BV_GANG")) { const int v = atoi(e); if (v >= 1) k.gang = v; }      // value: >= 1 overrides the planned gang size, else 0
		if (const char *e = getenv("GF2BV_BATCH_THREADS")) { const int v = atoi(e); if (v >= 1) k.batch_threads = std::min(v, 16); }      // value: min(v, 16) host threads of a batch call when v >= 1
		if (const char *e = getenv("GF2BV_SLAB_PAD")) k.slab_pad = std::max<i64>(1, atol(e));      // value, max(1, v), latched: rows behind a tile slab
		if (const char *e = getenv("GF2BV_KEEP_BIG")) k.keep_big = atoi(e) != 0;      // value, on, latched: 0 keeps no large idle buffer in the pool
		k.trace = getenv("GF2BV_TRACE") != nullptr;      // flag: host-side times on stderr
		if (const char *e = getenv("GF2BV_DEBUG_SYNC")) k.debug_sync = atoi(e);      // value, bit mask: hipDeviceSynchronize after every block's panel path (1) / bulk path (2)
		return k;
	}
	void refresh() { const Knobs now = read(); bs_inv = now.bs_inv; ysweep = now.ysweep; trace = now.trace; }      // a later call on a kept handle
	std::string dump() const          // one NAME=value line per variable, as parsed (gf2bv_knob_dump)
	{
		auto n = [](i64 v) { return std::to_string(v); };
		auto tri = [](int v) { return v < 0 ? std::string("unset") : std::to_string(v); };
		char mib[32]; snprintf(mib, sizeof mib, "%g", two_level_min_mib);
		const std::pair<const char *, std::string> rows[] = {
			{ "GF2BV_PLAIN", n(plain) }, { "GF2BV_STREAM_PAIRS", tri(stream_pairs) }, { "GF2BV_UPDATE", n(update) }, { "GF2BV_TWO_LEVEL", tri(two_level) },
			{ "GF2BV_TWO_LEVEL_MIN_MIB", two_level_min_set ? mib : "unset" }, { "GF2BV_OUTER_CHAIN", n(outer_chain) }, { "GF2BV_OUTER_SIDE", n(outer_side) },
			{ "GF2BV_FAST", n(fast) }, { "GF2BV_OPTIMISTIC", tri(optimistic) }, { "GF2BV_FUSED_NARROW", n(fused_narrow) }, { "GF2BV_SPARSE_FAST", n(sparse_fast) },
			{ "GF2BV_PC", n(pc) }, { "GF2BV_FLAG_SYNC", n(flag_sync) }, { "GF2BV_SERIAL", n(serial) }, { "GF2BV_XCD_PIN", tri(xcd_pin) }, { "GF2BV_XCD_WGS", n(xcd_wgs) },
			{ "GF2BV_GANG_NT", n(gang_nt) }, { "GF2BV_GANG_BS", n(gang_bs) }, { "GF2BV_BS_INV", tri(bs_inv) }, { "GF2BV_YSWEEP", n(ysweep) }, { "GF2BV_SMALL", n(small) },
			{ "GF2BV_SMALL_ZC", tri(small_zc) }, { "GF2BV_SMALL_PROBE", n(small_probe) }, { "GF2BV_SELF_WAIT_US", n(self_wait_us) }, { "GF2BV_GANG", n(gang) },
			{ "GF2BV_BATCH_THREADS", n(batch_threads) }, { "GF2BV_SLAB_PAD", n(slab_pad) }, { "GF2BV_KEEP_BIG", n(keep_big) }, { "GF2BV_HOST_POOL_MB", n(host_pool_mb) },
			{ "GF2BV_TRACE", n(trace) }, { "GF2BV_DEBUG_SYNC", n(debug_sync) },
		};
		std::string s;
		for (const auto &r : rows) s += std::string(r.first) + "=" + r.second + "\n";
		return s;
	}
};

struct Trace {
	std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	void mark(const Knobs &kn, const char *what)
	{
		if (!kn.trace) return;
		auto t = std::chrono::steady_clock::now();
		fprintf(stderr, "[gf2bv trace] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t0).count());
		t0 = t;
	}
};
// rows of one tile slab: the rows padded to a wavefront's 64, plus 64 more (>= 1 is needed: rows nobody owns take the outer
// pass's dummy stores).  A slab is then a whole number of KiB, and a wavefront's batch -- 64 consecutive rows of a 16-byte tile
// -- is eight whole 128-byte lines.  Rounds 1-2 padded by 2 rows ("skew neighbouring tiles across the channels": 32 bytes per
// tile with 16-byte tiles): every batch of every tile but the first then straddled NINE lines.  65536^2: 33.7 -> 32.5 ms with
// any multiple of 64 (64 ... 1024 alike: the channel hash does not care about the stride); other sizes 0-1 %
// (profiles/r03_slab_pad.txt; GF2BV_SLAB_PAD=2 restores the old layout).
inline i64 slab_pad() { static const i64 pad = Knobs::read().slab_pad; return pad; }
inline i64 slab_rows(i64 rows) { return round_up(std::max<i64>(rows, 1), 64) + slab_pad(); }
// column tiles of a row of wt words: whole ownership units of 8 words (one 64-byte tile / four 16-byte tiles)
inline i64 tiles_for(i64 wt) { return round_up(std::max<i64>(wt, 1), (i64)1 << GF2_OWN_LOG) / GF2_TW; }


// ---- resource pool -----------------------------------------------------------------------------
// hipMalloc / hipFree / stream and event creation cost 0.1-1 ms each; a small solve (a few hundred
// microseconds of GPU time) would spend 5+ ms in them.  Buffers up to 64 MiB (512 MiB in total per
// process), streams and events are therefore recycled across calls.  Thread-safe; everything handed
// out is idle (a solve releases its resources only after synchronising its streams).

struct Pool {
	std::mutex mu;
	std::unordered_map<void *, std::pair<int, size_t>> live;          // ptr -> (device, bucket bytes)
	std::map<std::pair<int, size_t>, std::vector<void *>> free_bufs;  // (device, bucket) -> buffers
	size_t cached_bytes = 0;
	std::map<std::pair<int, int>, std::vector<hipEvent_t>> events;   // (device, timing?) -> events
	std::map<std::pair<int, int>, std::vector<hipStream_t>> streams;  // (device, low priority?) -> streams
	static constexpr size_t kMaxBucket = (size_t)64 << 20, kMaxCached = (size_t)512 << 20;
	// A few LARGE buffers per device (the working matrices of the last big solves) are kept as well: hipMalloc +
	// hipFree of 2-8 GiB cost 10-100 ms per call, a visible part of a 0.3-2 s solve.  Up to kMaxBig of them (round 4: the
	// batch entry runs two or three gangs at a time, each with a working buffer of 3-4 GiB -- with ONE kept buffer every other
	// gang paid an allocation and a free).  Round 5: what is kept is bounded by the DEVICE (a sixth of its memory, 48 GiB at
	// most; GF2BV_KEEP_BIG=0: nothing is kept), an allocation that fails frees everything idle on that device and is
	// repeated once, gf2bv_pool_trim() does the same on request, and no hipFree runs under the pool's mutex.
	struct Big { void *p = nullptr; size_t bytes = 0; };
	static constexpr size_t kMaxBig = 6, kMaxBigBytes = (size_t)48 << 30;      // (a gang holds two: working matrices and the side-array arena)
	std::map<int, std::vector<Big>> big_free;                         // device -> idle large buffers
	std::unordered_map<void *, std::pair<int, size_t>> big_live;      // handed-out large buffers
	std::map<int, size_t> big_cap;                                    // device -> bytes of idle large buffers kept there
	static bool keep_big() { static const bool keep = Knobs::read().keep_big; return keep; }
	// (mu held) idle large buffers of `device` may hold this many bytes: a sixth of the device's memory, 48 GiB at most
	size_t big_cap_locked(int device)
	{
		auto it = big_cap.find(device);
		if (it != big_cap.end()) return it->second;
		size_t cap = kMaxBigBytes, fr = 0, total = 0;
		int cur = -1;
		(void)hipGetDevice(&cur);
		if (cur == device && hipMemGetInfo(&fr, &total) == hipSuccess && total) cap = std::min(cap, total / 6);
		else if (cur != device) return cap;       // (not the calling thread's device: ask again later)
		big_cap[device] = cap;
		return cap;
	}

	static size_t bucket(size_t bytes)
	{
		size_t b = 4096;
		while (b < bytes) b <<= 1;
		return b;
	}
	// every idle buffer of `device` (large ones and the bucket cache) leaves the pool; the caller frees them OUTSIDE the lock
	void take_idle_locked(int device, std::vector<void *> &drop)
	{
		auto bf = big_free.find(device);
		if (bf != big_free.end()) { for (const Big &b : bf->second) drop.push_back(b.p); bf->second.clear(); }
		for (auto &kv : free_bufs)
			if (kv.first.first == device) {
				for (void *q : kv.second) { drop.push_back(q); cached_bytes -= kv.first.second; }
				kv.second.clear();
			}
	}
	// gf2bv_pool_trim: returns the bytes given back to the device
	size_t trim(int device)
	{
		std::vector<void *> drop;
		size_t bytes = 0;
		{
			std::lock_guard<std::mutex> lk(mu);
			auto bf = big_free.find(device);
			if (bf != big_free.end()) for (const Big &b : bf->second) bytes += b.bytes;
			for (auto &kv : free_bufs) if (kv.first.first == device) bytes += kv.first.second * kv.second.size();
			take_idle_locked(device, drop);
		}
		for (void *q : drop) (void)hipFree(q);
		return bytes;
	}
	// hipMalloc; on out-of-memory everything idle on the device is freed and the allocation repeated once
	hipError_t malloc_retry(void **out, size_t bytes, int device)
	{
		hipError_t e = hipMalloc(out, bytes);
		if (e != hipErrorOutOfMemory) return e;
		(void)hipGetLastError();
		if (trim(device) == 0) return e;
		return hipMalloc(out, bytes);
	}
	hipError_t alloc(void **out, size_t bytes, int device)
	{
		bytes = std::max<size_t>(bytes, 16);
		if (bytes > kMaxBucket) {
			void *stale = nullptr;
			{
				std::lock_guard<std::mutex> lk(mu);
				auto &v = big_free[device];
				for (size_t i = 0; i < v.size(); i++)
					if (v[i].bytes >= bytes && v[i].bytes <= bytes + bytes / 2) {
						*out = v[i].p; big_live[v[i].p] = {device, v[i].bytes};
						v.erase(v.begin() + i);
						return hipSuccess;
					}
				if (v.size() >= kMaxBig) { stale = v.front().p; v.erase(v.begin()); }     // none fits: make room (the oldest goes) before allocating
			}
			if (stale) (void)hipFree(stale);
			hipError_t e = malloc_retry(out, bytes, device);
			if (e == hipSuccess && keep_big()) { std::lock_guard<std::mutex> lk(mu); big_live[*out] = {device, bytes}; }
			return e;
		}
		const size_t b = bucket(bytes);
		{
			std::lock_guard<std::mutex> lk(mu);
			auto &v = free_bufs[{device, b}];
			if (!v.empty()) {
				*out = v.back(); v.pop_back(); cached_bytes -= b;
				live[*out] = {device, b};
				return hipSuccess;
			}
		}
		hipError_t e = malloc_retry(out, b, device);
		if (e == hipSuccess) { std::lock_guard<std::mutex> lk(mu); live[*out] = {device, b}; }
		return e;
	}
	void release(void *p)
	{
		if (!p) return;
		std::vector<void *> drop;          // freed after the lock is gone: hipFree of a multi-GiB buffer synchronises the device
		{
			std::lock_guard<std::mutex> lk(mu);
			auto bl = big_live.find(p);
			auto it = live.find(p);
			if (bl != big_live.end()) {
				const int device = bl->second.first;
				const size_t bytes = bl->second.second;
				big_live.erase(bl);
				auto &v = big_free[device];
				Big nb; nb.p = p; nb.bytes = bytes;
				v.push_back(nb);
				size_t sum = 0;
				for (const Big &b : v) sum += b.bytes;
				const size_t cap = big_cap_locked(device);
				while (!v.empty() && (v.size() > kMaxBig || sum > cap)) { sum -= v.front().bytes; drop.push_back(v.front().p); v.erase(v.begin()); }     // the oldest go
			}
			else if (it != live.end()) {
				const auto key = it->second;
				live.erase(it);
				if (cached_bytes + key.second <= kMaxCached) { free_bufs[key].push_back(p); cached_bytes += key.second; }
				else drop.push_back(p);
			}
			else drop.push_back(p);
		}
		for (void *q : drop) (void)hipFree(q);
	}
	// streams and events handed out and not yet returned, per device (gf2bv_pool_in_use; the buffers are `live` and `big_live`)
	std::map<int, i64> streams_out, events_out;
	hipError_t event(hipEvent_t *e, bool timing)
	{
		int device = 0;
		(void)hipGetDevice(&device);
		{
			std::lock_guard<std::mutex> lk(mu);
			auto &v = events[{device, timing ? 1 : 0}];
			if (!v.empty()) { *e = v.back(); v.pop_back(); events_out[device]++; return hipSuccess; }
		}
		const hipError_t err = timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming);
		if (err == hipSuccess) { std::lock_guard<std::mutex> lk(mu); events_out[device]++; }
		return err;
	}
	void release_event(hipEvent_t e, bool timing)
	{
		if (!e) return;
		int device = 0;
		(void)hipGetDevice(&device);
		std::lock_guard<std::mutex> lk(mu);
		events_out[device]--;
		auto &v = events[{device, timing ? 1 : 0}];
		if (v.size() < 8192) v.push_back(e); else (void)hipEventDestroy(e);
	}
	// cls: 0 = normal priority, 1 = low priority (the bulk side of a solve); + 2 = the same for BATCH calls and their gangs.  The two
	// worlds do not trade streams (round 5): which low-priority stream a single solve finds on top of the pool decides whether it runs
	// 5.4 or 12.7 ms (low_stream_for below), and batch calls with several host threads return their streams in any order.
	hipError_t stream(hipStream_t *s, int device, int cls)
	{
		const bool low = cls & 1;
		{
			std::lock_guard<std::mutex> lk(mu);
			auto &v = streams[{device, cls}];
			if (!v.empty()) { *s = v.back(); v.pop_back(); streams_out[device]++; return hipSuccess; }
		}
		int lo = 0, hi = 0;
		if (low) (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
		const hipError_t err = low ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, lo) : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
		if (err == hipSuccess) { std::lock_guard<std::mutex> lk(mu); streams_out[device]++; }
		return err;
	}
	void release_stream(hipStream_t s, int device, int cls)
	{
		if (!s) return;
		std::lock_guard<std::mutex> lk(mu);
		streams_out[device]--;
		streams[{device, cls}].push_back(s);
	}
	// A low-priority stream for the bulk side of a solve whose panel path runs on `a` (round 5).  Not every pair of streams is equal on
	// this chip: with some pairs the workgroups of a kernel on `a` are handed out at ~0.4 us apiece while a chip-filling kernel on the
	// other stream has its successor queued behind it -- 80 workgroups take 37 us instead of 3 -- and a latency-bound solve (MT19937
	// recovery, 78 blocks) runs 12.7 ms instead of 5.4: panel path and bulk path end up one after the other.  Which pairs: a property of
	// the two streams (the hardware queues behind them), stable for the life of the process, the same for every solve -- seen as "the
	// single solves after a batch call are slow this time": the batch had left another of its streams on top of the pool
	// (profiles/r05_stream_pairs.txt).  So a pair is probed once (two holds with the bulk update's footprint on the candidate, a
	// one-workgroup and an 80-workgroup kernel with a panel kernel's footprint on `a`: when did the last of the 80 begin) and the
	// verdict kept; idle streams known to be good with `a` are preferred, unknown ones probed, at most kMaxLow low-priority streams per
	// device are created, and when nothing passes the first candidate is taken as it is.  GF2BV_STREAM_PAIRS=0: any idle stream.
	static constexpr int kMaxLow = 10;
	std::mutex probe_mu;                                                  // one probe at a time (it wants the queues to itself)
	std::map<std::pair<hipStream_t, hipStream_t>, int> pair_ok;           // (panel stream, low-priority stream) -> 1 good, 0 throttled
	std::map<int, int> low_created;                                       // device -> low-priority streams created so far
	int pairs_probed = 0, pairs_bad = 0;
	// The probe: a miniature of a solve's pattern, NB "blocks".  Panel stream: two one-workgroup kernels with a panel kernel's footprint
	// (256 threads, 23 KiB of LDS) that work 10 us each, then a flag; bulk stream: a gate on that flag, then a chip-filling kernel with the
	// bulk update's footprint (512 threads and 133 KiB per CU) that holds 40 us.  The panel chain depends on nothing the bulk stream
	// does: on a good pair it ends after NB x ~24 us (measured 187-192 us for 8 blocks), on a bad one after NB x ~55 us (439-446): each
	// block's panel kernels wait for the hold before them.  (A first probe -- when does the last of 80 panel-shaped workgroups begin
	// beside two holds: 3 us or 36 -- saw only some of the bad pairs; this one agreed with the solve on 38 of 38 pairs.)
	hipError_t probe_pair(hipStream_t a, hipStream_t b, int device, int *ok, const Knobs &kn);
	// cls: the class the stream comes from and goes back to (1, or 3 for a batch call's gangs); also: the panel streams of the solves that
	// will run beside this one (all idle now) -- the stream has to get on with them as well.
	hipError_t low_stream_for(const Knobs &kn, hipStream_t a, int device, hipStream_t *out, int cls = 1, const std::vector<hipStream_t> &also = {})
	{
		if (!(kn.stream_pairs >= 0 ? kn.stream_pairs != 0 : !kn.plain) || !a) return stream(out, device, cls);
		std::lock_guard<std::mutex> pl(probe_mu);
		std::vector<hipStream_t> rejected, with;
		with.push_back(a);
		for (hipStream_t x : also) if (x && x != a) with.push_back(x);
		hipError_t err = hipSuccess;
		*out = nullptr;
		// verdict of candidate c against everything in `with`, as far as known: 1 all good, 0 one throttled, -1 something unknown
		auto known = [&](hipStream_t c) {
			int r = 1;
			for (hipStream_t x : with) {
				auto it = pair_ok.find({x, c});
				if (it == pair_ok.end()) r = r == 0 ? 0 : -1; else if (it->second == 0) r = 0;
			}
			return r;
		};
		for (int attempt = 0; attempt < kMaxLow + 2 && !*out; attempt++) {
			hipStream_t c = nullptr;
			bool known_good = false;
			{
				std::lock_guard<std::mutex> lk(mu);
				auto &v = streams[{device, cls}];
				for (size_t i = v.size(); i-- > 0 && !c;)
					if (known(v[i]) == 1) { c = v[i]; v.erase(v.begin() + (ptrdiff_t)i); known_good = true; }
				for (size_t i = v.size(); i-- > 0 && !c;)
					if (known(v[i]) == -1) { c = v[i]; v.erase(v.begin() + (ptrdiff_t)i); }
				if (!c) {
					if (low_created[device] >= kMaxLow) break;
					low_created[device]++;
				}
				else streams_out[device]++;             // (a rejected candidate goes back through release_stream)
			}
			if (known_good) { *out = c; break; }
			if (!c) {
				int lo = 0, hi = 0;
				(void)hipDeviceGetStreamPriorityRange(&lo, &hi);
				if ((err = hipStreamCreateWithPriority(&c, hipStreamNonBlocking, lo)) != hipSuccess) break;
				std::lock_guard<std::mutex> lk(mu);
				streams_out[device]++;
			}
			int all_ok = 1;
			for (hipStream_t x : with) {
				int ok = -1;
				{
					std::lock_guard<std::mutex> lk(mu);
					auto it = pair_ok.find({x, c});
					if (it != pair_ok.end()) ok = it->second;
				}
				if (ok < 0) {
					ok = 1;
					if (probe_pair(x, c, device, &ok, kn) != hipSuccess) { (void)hipGetLastError(); ok = 1; }      // (a probe that cannot run decides nothing -- and leaves no verdict: the pair is asked again)
					else {
						std::lock_guard<std::mutex> lk(mu);
						pair_ok[{x, c}] = ok;
						pairs_probed++; pairs_bad += !ok;
					}
				}
				if (!ok) { all_ok = 0; break; }
			}
			if (all_ok) *out = c; else rejected.push_back(c);
		}
		if (!*out && !rejected.empty()) { *out = rejected.front(); rejected.erase(rejected.begin()); }
		for (hipStream_t r : rejected) release_stream(r, device, cls);
		if (!*out && err == hipSuccess) return stream(out, device, cls);
		return err;
	}
};
Pool &pool()
{
	static Pool *p = new Pool();      // intentionally leaked: the HIP runtime may be gone at static destruction
	return *p;
}
// A pool buffer for an entry that tells "does not fit" from a failure: out of device memory is GF2BV_ERR_NOMEM with the message
// `nomem` (and the runtime's sticky error cleared), any other error GF2BV_ERR_HIP with `what`.
int nomem_or_hip(hipError_t e, const char *nomem, const char *what)
{
	if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(GF2BV_ERR_NOMEM, nomem); }
	if (e != hipSuccess) return fail(GF2BV_ERR_HIP, what, e);
	return GF2BV_OK;
}
// (a buffer that a Solver or a kept handle owns: not scope-held)
int alloc_or_nomem(void **out, size_t bytes, int device, const char *nomem, const char *what) { return nomem_or_hip(pool().alloc(out, bytes, device), nomem, what); }

// What one scope borrows from the pool: at most one stream -- the pool's, of class `cls`, or the caller's, which is waited for and
// never returned -- and any number of buffers and events.  THE rule of giving back, on every return path (every HIPCHK is an early
// return, and work may be in flight then): the stream and every stream named with wait_for() are synchronised, then the buffers go
// back, then the events, then the stream, to the class it came from.
struct Held {
	const int device;
	hipStream_t st = nullptr;
	explicit Held(int device) : device(device) {}
	Held(int device, hipStream_t callers) : device(device) { on(callers); }
	Held(const Held &) = delete;
	~Held()
	{
		for (hipStream_t s : waits) (void)hipStreamSynchronize(s);
		for (void *p : bufs) pool().release(p);
		for (const auto &e : events) pool().release_event(e.first, e.second);
		if (cls >= 0) pool().release_stream(st, device, cls);
	}
	hipError_t stream(int from_cls)                // a stream of the pool
	{
		const hipError_t e = pool().stream(&st, device, from_cls);
		if (e == hipSuccess) { cls = from_cls; waits.push_back(st); }
		return e;
	}
	void on(hipStream_t callers) { st = callers; waits.push_back(st); }       // (null: the null stream)
	void wait_for(hipStream_t s) { waits.push_back(s); }
	hipError_t get(void **out, size_t bytes)
	{
		const hipError_t e = pool().alloc(out, bytes, device);
		if (e == hipSuccess) bufs.push_back(*out);
		return e;
	}
	int alloc(void **out, size_t bytes, const char *nomem, const char *what) { return nomem_or_hip(get(out, bytes), nomem, what); }
	hipError_t event(hipEvent_t *ev, bool timing = true)
	{
		const hipError_t e = pool().event(ev, timing);
		if (e == hipSuccess) events.push_back({ *ev, timing });
		return e;
	}
private:
	int cls = -1;                                  // the pool class `st` goes back to; -1: not the pool's
	std::vector<hipStream_t> waits;
	std::vector<void *> bufs;
	std::vector<std::pair<hipEvent_t, bool>> events;
};

hipError_t Pool::probe_pair(hipStream_t a, hipStream_t b, int device, int *ok, const Knobs &kn)
{
	*ok = 1;
	constexpr int NB = 6;
	constexpr double limit_us = 37.0 * NB;
	unsigned long long *q = nullptr, hq[2 * NB + 2];
	int *fl = nullptr;
	Held H(device, a); H.wait_for(b);
	hipError_t e;
	auto bad = [&](hipError_t x) { return (e = x) != hipSuccess; };
	if (bad(H.get((void **)&q, sizeof hq)) || bad(H.get((void **)&fl, sizeof(int) * 2 * NB))) return e;
	int cus = 256;
	(void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
	auto measure = [&](double *chain_us) -> hipError_t {
		if (bad(hipMemsetAsync(fl, 0, sizeof(int) * 2 * NB, a)) || bad(hipMemsetAsync(q, 0, sizeof hq, a))) return e;
		if (bad(hipStreamSynchronize(a)) || bad(hipStreamSynchronize(b))) return e;
		k_probe_stamp_panel<<<dim3(1), dim3(256), 0, a>>>(q + 2 * NB);
		for (int i = 0; i < NB; i++) {
			k_probe_panel_work<<<dim3(1), dim3(256), 0, a>>>(q + 2 * i, 1000ull);
			k_probe_panel_work<<<dim3(1), dim3(256), 0, a>>>(q + 2 * i + 1, 1000ull);
			k_probe_set<<<dim3(1), dim3(1), 0, a>>>(fl + i);
			k_probe_wait<<<dim3(1), dim3(1), 0, b>>>(fl + i, fl + NB + i, 200000ull);
			k_probe_hold_bulk<<<dim3((unsigned)cus), dim3(512), 0, b>>>(q + 2 * NB + 1, 4000ull);
		}
		if (bad(hipGetLastError()) || bad(hipStreamSynchronize(a)) || bad(hipStreamSynchronize(b))) return e;
		if (bad(hipMemcpy(hq, q, sizeof hq, hipMemcpyDeviceToHost))) return e;
		*chain_us = ((double)hq[2 * NB - 1] - (double)hq[2 * NB]) / 100.0;
		return hipSuccess;
	};
	// a verdict near the threshold (good pairs measure ~24 us per probe block, bad ones ~55: other work on the device can push a
	// probe either way) is not kept on one sample: the pair is measured again, three times in all at most, and the FASTER run
	// decides -- a neighbour can only slow a probe down.  A repeat that cannot run decides nothing.
	bool good = false;
	for (int k = 0; k < 3; k++) {
		double chain_us = 0;
		if (bad(measure(&chain_us))) {
			if (k == 0) return e;
			(void)hipGetLastError();
			break;
		}
		good = good || chain_us < limit_us;
		if (kn.trace)
			fprintf(stderr, "[gf2bv trace] stream pair %p / %p: the panel chain of %d probe blocks took %.1f us (%s)\n", (void *)a, (void *)b, NB, chain_us,
			        chain_us < limit_us ? "good" : "waits for the bulk stream");
		if (!(chain_us > 0.75 * limit_us && chain_us < 1.5 * limit_us)) break;
	}
	*ok = good;
	return hipSuccess;
}

// ---- kernel configurations -----------------------------------------------------------------
// Bulk update: G panels fused per HBM pass, T grease tables per panel (balanced bit-fields).
int streams_run_concurrently(const Knobs &kn, int device, hipStream_t a, hipStream_t b, int *ok);
int xcd_dispatch_is_round_robin(int device, hipStream_t st, int *ok);
void forget_concurrency(int device);

struct UpdateImpl {
	int G, T, lds_bytes, threads;
	hipError_t (*update)(dim3, hipStream_t, u64 *, i64, i64, int, int, int, const PanelRec *, const PanelAux *,
	                     const u64 *, const int *, int, int, int, int, int, bool, const uint4 *, SysStride, hipEvent_t, hipEvent_t, int,
	                     unsigned long long *, unsigned long long *);
};

// 16-byte tiles: G = 4 panels, T = 8 byte fields per panel.  nw_lo < 0 selects the HALF instance (only the tile's second
// word is stored: its first one belongs to the next block's window); the window's whole tiles are simply not launched.
template <int NT, int DEPTH, bool PIPE, int LB>
hipError_t launch_update16(dim3 grid, hipStream_t s, u64 *M, i64 rows, i64 srows, int j0, int gb, int wlo,
                           const PanelRec *panels, const PanelAux *aux, const u64 *multset, const int *blk_first,
                           int tile_begin, int ntiles, int world, int wrank, int nw_lo, bool stream_rows, const uint4 *Pc, SysStride ss,
                           hipEvent_t begun, hipEvent_t done, int xcd_nsys, unsigned long long *t_first, unsigned long long *t_last)
{
	if (xcd_nsys > 0) grid = dim3(grid.x * grid.y);          // one line of workgroups, decoded in the kernel (a system per XCD)
	{
		// stream_rows: streaming (non-temporal) row accesses -- pinned gangs (GF2BV_GANG_NT=0: plain).  The streaming form exists for the
		// default instance only: with GF2BV_UPDATE != 0 the selected instance runs with plain accesses.
		if (stream_rows && NT == 512 && DEPTH == 3 && PIPE && LB == 512) {
			if (nw_lo < 0)
				hipExtLaunchKernelGGL((k_update16<512, true, 3, true, 512, true>), grid, dim3(512), 0, s, begun, done, 0, M, rows, srows, j0, gb, wlo,
				                      panels, aux, multset, blk_first, tile_begin, ntiles, world, wrank, Pc, ss, xcd_nsys, t_first, t_last);
			else
				hipExtLaunchKernelGGL((k_update16<512, false, 3, true, 512, true>), grid, dim3(512), 0, s, begun, done, 0, M, rows, srows, j0, gb, wlo,
				                      panels, aux, multset, blk_first, tile_begin, ntiles, world, wrank, Pc, ss, xcd_nsys, t_first, t_last);
			return hipGetLastError();
		}
	}
	if (nw_lo < 0)
		hipExtLaunchKernelGGL((k_update16<NT, true, DEPTH, PIPE, LB>), grid, dim3(NT), 0, s, begun, done, 0, M, rows, srows, j0, gb, wlo,
		                      panels, aux, multset, blk_first, tile_begin, ntiles, world, wrank, Pc, ss, xcd_nsys, t_first, t_last);
	else
		hipExtLaunchKernelGGL((k_update16<NT, false, DEPTH, PIPE, LB>), grid, dim3(NT), 0, s, begun, done, 0, M, rows, srows, j0, gb, wlo,
		                      panels, aux, multset, blk_first, tile_begin, ntiles, world, wrank, Pc, ss, xcd_nsys, t_first, t_last);
	return hipGetLastError();
}
#define UPDATE16_IMPL(NT, D, P, LB) { 4, 8, 2 * 256 * 256 + GF2_GMAX * 64 * 20, NT, launch_update16<NT, D, P, LB> }

const UpdateImpl kUpdates[] = {
	// default: 8 wavefronts (two per SIMD, 157 VGPRs: three batches of 64 rows in flight per wavefront, the lookups of
	// round r+1 issued before the XORs of round r); the kernel is bound by the memory side, so more wavefronts buy
	// nothing (65536^2 / 131072^2 wall: 37.8 / 212.9 ms; 12 wavefronts 38.4 / 212.5; 16: 40.7 / 221) and half of every
	// SIMD's registers plus 27 KiB of LDS stay free for the panel kernels of the next block
	UPDATE16_IMPL(512, 3, true, 512),
	UPDATE16_IMPL(768, 2, true, 768),
	UPDATE16_IMPL(768, 2, true, 1024),
	UPDATE16_IMPL(1024, 2, false, 1024),
	UPDATE16_IMPL(768, 3, true, 768),
	UPDATE16_IMPL(640, 2, true, 640),
};

static_assert(sizeof kUpdates / sizeof kUpdates[0] == Knobs::kNumUpdates, "GF2BV_UPDATE indexes this table");

// Back-substitution sweeps over Y use the single-panel kernel (5-bit tables, 128-byte segments).
constexpr int YK = 5, YTW = 16, YNT = 1024;
hipError_t launch_ysweep(dim3 grid, hipStream_t s, u64 *Y, i64 ys, i64 rows, const PanelRec *rec,
                         const u64 *mult, int ntiles, int rpb)
{
	constexpr int lds = SweepCfg<YK, YTW>::LDS_BYTES;
	static std::mutex attr_mu;
	static std::map<int, bool> attr_set;          // device -> the > 64 KiB dynamic-LDS attribute has been raised there
	int dev = 0;
	(void)hipGetDevice(&dev);
	{
		std::lock_guard<std::mutex> lk(attr_mu);
		if (!attr_set[dev]) {
			hipError_t e = hipFuncSetAttribute((const void *)k_sweep<YK, YTW, YNT>,
			                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds);
			if (e != hipSuccess) return e;
			attr_set[dev] = true;
		}
	}
	k_sweep<YK, YTW, YNT><<<grid, dim3(YNT), lds, s>>>(Y, ys, rows, rec, 1, mult, 0, ntiles, rpb);
	return hipGetLastError();
}

constexpr int TW = GF2_TW;        // words per column tile

// ---- one solve ---------------------------------------------------------------------------------
inline size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Where the side arrays of ONE system lie in its arena: byte offsets, each rounded up to 256, in this order (solver_alloc clears
// st .. died and blk_first .. Wb with one memset each), and the bytes from one system of a gang to the next.  arena_layout()
// computes it, ArenaPtrs::bind() turns it into pointers; nothing else lists the members.
struct ArenaLayout {
	size_t st = 0, sf = 0, panels = 0, aux = 0, fu = 0, died = 0, pivcol = 0, urow = 0, blk_first = 0, mult = 0, Wb = 0, Uwin = 0, Pfast = 0,
	       oprow = 0, Tm = 0, Pc = 0, wmask = 0, stride = 0;
};

// The three ways a block goes down the panel stream (enqueue_block_panel; block_way picks one):
//   General      the G + 1 general panel steps, the dense one-launch search in front of them where fast_block_possible
//   DenseOnly    k_block_fast + the one-pass narrow step only (or the two fused: k_block_fast_narrow)
//   SparseOnly   k_block_sparse + the one-pass narrow step only
enum class BlockWay { General, DenseOnly, SparseOnly };

// What changes while the forward pass of a solve is being enqueued: which one-launch search the blocks get, and what the host has
// learnt from the blocks a search handed back.  One pass per Solver, so the initial values are the pass's.
struct ForwardRun {
	// Optimistic enqueue for dense systems: block 0 took the dense search, so the blocks that can take it at all get it alone
	bool dense_only = false;
	// Sparse systems (round 5): blocks the dense one-launch search cannot take go through k_block_sparse -- candidates = the alive rows
	// with a non-zero window, from the bit masks the look-ahead leaves in wmask (allowed at all: kn.sparse_fast)
	bool sparse_on = false;       // this solve has switched to it (after block 0 went the general way)
	int tier = 0;                 // pool size of k_block_sparse, an index into kSparsePools: 0 = 1024 rows (beside the bulk update), 1 = 4096, 2 = 6144
	int giveups = 0, why[5] = {}; // blocks handed back to the general steps (gf2bv_stats::sparse_giveups), and by the kernel's reason 1..5 (SolveState::sp_why)
	// the first block of each pool size is looked at before anything is enqueued behind it: a pool that cannot serve the system (too
	// many rows carry a bit in a window) costs one block, not a poisoned pipeline of all the blocks behind it
	int probes = 1;
	int general_only = -1;        // (after a hand-back) this one block takes the general steps whatever the mode
};

// What a solve IS apart from the device and pool resources it holds: the shape, the plan, the counters and the host copies.  Plain
// values, free to copy -- a gang's views and the copy of a kept factorization start from their original's (make_view, factor_copy).
struct SolverPlan {
	int device = 0;
	i64 rows = 0, cols = 0, stride = 0;
	i64 ntiles = 0, srows = 0;    // tiles, rows per tile slab (padded)
	// gang: nsys same-shape systems eliminated in lock-step by the same launches (blockIdx.y = system);
	// system s lives at M + s * m_stride words / arena + s * lay.stride bytes, its input at src + s * src_sys_words
	int nsys = 1;
	int gang_nsys = 1;            // (a view: the size of the gang it belongs to)
	// column-slab solve of ONE system over `world` GPUs: this rank owns the column tiles t with t % world == wrank
	// (cyclic, so that the shrinking trailing matrix stays balanced) and runs the bulk path on those only; the panel
	// path of a block runs on the owner of its window's tile (see gf2bv_slab_* below)
	int world = 1, wrank = 0;
	i64 m_stride = 0, src_sys_words = 0;
	ArenaLayout lay;              // (a view: of its one system, stride 0)
	bool view = false;            // a non-owning window on one system of a gang (back-substitution, export)
	SysStride ss() const { return SysStride{ m_stride, (i64)lay.stride }; }
	int mode = 0;
	// many right-hand sides of one matrix (gf2bv_solve_rhs_*): right-hand side j is column cols + j, k_check_rhs_many leaves
	// the per-RHS inconsistency bits in rhs_bad (ceil(nrhs / 64) words); nrhs == 1 with rhs_bad == nullptr: every other entry
	int nrhs = 1;
	bool time_kernels = false;
	Knobs kn;                     // the environment switches as solver_alloc found them (see Knobs: a kept handle refreshes three per call)
	const UpdateImpl *impl = nullptr;

	int nsets = 2;                // multiplier sets (ArenaPtrs::mult)
	// two-level elimination (large systems; see k_update16k): blocks [0, tl_bend) go in outer panels of tl_K blocks
	int tl_K = 0, tl_bend = 0;
	i64 tile_hi = 0;              // bulk kernels touch tiles < tile_hi (= ntiles; the outer panel's end while it is eliminated)
	static constexpr int nlist = 2;      // row lists / T matrices kept: by panel parity (the previous panel's outer pass may still be reading its own)
	bool bulk_waits_outer = false;     // the next bulk launch of the one-level schedule has to wait for the last outer pass
	bool ends_outer_panel(int b) const { return tl_K > 0 && b < tl_bend && (b + 1) % tl_K == 0; }
	// what a solve decides from the switches and the device (set in one block of solver_alloc)
	bool flag_sync = true;        // per-block hand-overs between the streams through sf + k_gate instead of events (kn.flag_sync; the device has a say)
	bool optimistic = true;       // the general panel steps are dropped behind the one-launch search once block 0 has taken it (kn.optimistic)
	bool xcd_pin = true;          // gangs of a multiple of 8 systems: every system's bulk-update workgroups on ONE XCD, one system after the other, with
	                              // streaming row accesses (single systems keep plain ones: measured <= 1 % either way in round 4); false: the plain grid
	int sync_base = 0;            // the counters only grow: a pass that re-enqueues blocks (resume after a poisoned one) counts from here
	int units = 0;
	ForwardRun run;               // what the forward pass decides while it is enqueued (fill_stats and the look-ahead read it)
	int narrow_rpt = 1;           // row blocks of 256 per narrow workgroup of a panel step (set in solver_alloc)
	i64 maxr = 0;
	int npanels = 0, nblocks = 0;
	i64 wt = 0, cw = 0;

	std::vector<int> free_order;     // free columns in M4RI kernel order (mode 1)
	// host staging of the export (filled by asynchronous copies between finish_begin and finish_end)
	SolveState hst{};
	std::vector<u64> hout;
	std::vector<PanelRec> hp;
	std::vector<int32_t> hpiv;
	std::chrono::steady_clock::time_point t_begin;
	float ms_pack = 0;
};

ArenaLayout arena_layout(const SolverPlan &P)
{
	const i64 R = std::max<i64>(1, P.rows), NP = std::max(1, P.npanels);
	const int G = P.impl->G;
	ArenaLayout L;
	size_t off = 0;
	auto carve = [&](size_t bytes) { size_t at = off; off += round256(bytes); return at; };
	L.st = carve(sizeof(SolveState)); L.sf = carve(sizeof(SyncFlags)); L.panels = carve(sizeof(PanelRec) * NP); L.aux = carve(sizeof(PanelAux) * NP);
	L.fu = carve(sizeof(FindUnit) * (P.units + 1 + GF2_MAXGROUPS)); L.died = carve(sizeof(int) * (size_t)R);
	L.pivcol = carve(sizeof(int) * (P.maxr + 64)); L.urow = carve(sizeof(int) * (P.maxr + 64));
	L.blk_first = carve(sizeof(int) * std::max(1, P.nblocks)); L.mult = carve(sizeof(u64) * P.nsets * G * mult_rows(R) + (P.tl_K ? kOuterSlackBytes : 0));
	L.Wb = carve(sizeof(u64) * 2 * GF2_GMAX * R); L.Uwin = carve(sizeof(u64) * GF2_GMAX * (P.maxr + 64));
	L.Pfast = carve(sizeof(u64) * GF2_GMAX * GF2_GMAX * 64); L.oprow = carve(sizeof(int) * GF2_OUTER_LISTS * P.nlist);
	L.Tm = carve(P.tl_K ? P.nlist * sizeof(u64) * GF2_KMAX * GF2_KMAX * GF2_GMAX * 64 * GF2_GMAX : 0);
	L.Pc = carve(P.kn.pc ? sizeof(u64) * 2 * GF2_GMAX * 64 * (size_t)P.ntiles : 0);
	L.wmask = carve(sizeof(u64) * 2 * (size_t)((R + 63) / 64 + 1));
	L.stride = off;
	return L;
}

// The side arrays of one system: pointers into its arena, set by bind() alone -- to a solve's fresh arena, to a view's part of its
// gang's, to the arena of a kept factorization's copy (whose `died` then moves to the handle's own died_buf where it has one).
struct ArenaPtrs {
	SolveState *st = nullptr;
	SyncFlags *sf = nullptr;      // progress counters of the two streams (k_gate)
	PanelRec *panels = nullptr;
	PanelAux *aux = nullptr;
	FindUnit *fu = nullptr;
	int *died = nullptr;          // per row: panel that made it a pivot source, GF2_NEVER while alive
	int *pivcol = nullptr, *urow = nullptr, *blk_first = nullptr;
	u64 *mult = nullptr;          // nsets sets x G x rows: block b writes / reads set b % nsets (2 = ping-pong; an outer panel of the
	                              // two-level elimination keeps all its K blocks' multipliers until its outer pass: nsets = K)
	u64 *Wb = nullptr;            // 2 x rows x GMAX window words (the panel steps ping-pong between the halves)
	u64 *Uwin = nullptr;          // rank x GMAX: pivot rows' words of the following window (k_prio_window -> k_unwind)
	u64 *Pfast = nullptr;         // scratch of k_block_fast: the pivot rows' window words of a block, [panel][word][column]
	int *oprow = nullptr;         // k_outer_prow -> k_outer_apply / k_update16k: row lists of the outer panel being applied
	u64 *Tm = nullptr;            // k_outer_trsm<IDENT> -> k_outer_apply: the panel's pivot rows as combinations of its source rows
	u64 *Pc = nullptr;            // final pivot rows of the current block, compact: [tile][panel][pivot bit] x 16 B (k_block_trsm -> k_update16); null: kn.pc is off
	u64 *wmask = nullptr;         // 2 x ceil(rows / 64) words: alive / alive with a non-zero window, per 64 rows

	void bind(const ArenaLayout &L, void *arena, bool pc)
	{
		char *base = (char *)arena;
		st = (SolveState *)(base + L.st); sf = (SyncFlags *)(base + L.sf); panels = (PanelRec *)(base + L.panels); aux = (PanelAux *)(base + L.aux);
		fu = (FindUnit *)(base + L.fu); died = (int *)(base + L.died); pivcol = (int *)(base + L.pivcol); urow = (int *)(base + L.urow);
		blk_first = (int *)(base + L.blk_first); mult = (u64 *)(base + L.mult); Wb = (u64 *)(base + L.Wb); Uwin = (u64 *)(base + L.Uwin);
		Pfast = (u64 *)(base + L.Pfast); oprow = (int *)(base + L.oprow); Tm = (u64 *)(base + L.Tm);
		Pc = pc ? (u64 *)(base + L.Pc) : nullptr;
		wmask = (u64 *)(base + L.wmask);
	}
};

// What one back-substitution on a Solver owns or borrows, and its shape.  backsub_begin() alone fills it (a gang's view: borrow());
// release() alone gives it back -- at the next begin, where a kept handle is done with a pass, or with the Solver.
struct BackSub {
	std::vector<int> cols;        // the columns solved for, ny of them: ycols is uploaded from here, so it lives as long as the copy may
	int *ycols = nullptr;
	u64 *out = nullptr;           // the solutions, max(1, cw) words each: one per column (a gang: one per system)
	u64 *Y = nullptr;             // Y sweeps: the selected columns of U as a bit matrix, ys words per pivot; parity chain: the diagonal blocks of U
	u64 *Minv = nullptr;          // inverted diagonal blocks (k_bs_inv -> k_bs_near2)
	int ny = 0;
	i64 ys = 0;
	bool borrowed = false;        // (a view) `out` points into its gang's: nothing here is this one's to return
	bool held() const { return ycols || out || Y || Minv; }
	void borrow(const BackSub &gang, int s, i64 cwx) { out = gang.out + (i64)s * cwx; ny = 1; borrowed = true; }
	// nothing goes back to the pool while the chain on sA may still be using it
	void release(hipStream_t sA)
	{
		if (held() && sA) (void)hipStreamSynchronize(sA);
		if (!borrowed) for (void *p : { (void *)Y, (void *)ycols, (void *)out, (void *)Minv }) pool().release(p);
		*this = BackSub();
	}
};

// The device and pool resources a solve holds (or, a view, borrows), the flags that say whose they are and the caller's own src and
// rhs_bad: never copied with the plan; Solver::release() alone gives back what is owned and resets the rest.
struct SolverHandles {
	hipStream_t sA = nullptr, sB = nullptr;      // panel path / bulk path
	bool own_sA = false, own_sB = false;
	u64 *M = nullptr;             // tile-major working copy (owned, unless ext_M)
	bool ext_M = false;           // the working matrix belongs to the caller (slab solves: a tensor the ranks exchange tiles of)
	const u64 *src = nullptr;     // caller's row-major matrix on the device (stride words per row)
	u64 *tmp_src = nullptr;       // row-major staging buffer when the input came from the host
	u64 *rhs_bad = nullptr;       // (the caller's: see nrhs)
	void *arena = nullptr;        // the side arrays of all nsys systems (ArenaPtrs: those of system 0)
	hipStream_t sC = nullptr;     // outer passes: panel p's runs BESIDE the inner elimination of panel p + 1 (sA + sB)
	                              // (late round 5 also split the pass itself over two streams, behind a switch of its own: 131072^2 162 -> 155 ms,
	                              // 262144^2 -0.8 %, but a fourth stream that cost later batch calls of the process their overlap; removed in
	                              // round 6, profiles/r05_outer_shapes.txt)
	hipEvent_t evOuter = nullptr, evPri = nullptr, evPanelDone = nullptr, evBig = nullptr;
	BackSub bs;                   // the back-substitution in flight, if any
	hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
	std::vector<hipEvent_t> evA, evPrio, kev, waitPrio;     // waitPrio[b]: the event that means "bulk of block b complete"
	hipEvent_t evx = nullptr;
	// time_kernels: the bulk-update launches stamp the clock themselves (k_update16: t_first / t_last) -- first[0] is the clock at
	// ev0, launch i owns first[i] and last[i] = stamps[stamp_cap + i].  kev keeps the launches that have no slot: the outer passes
	// of a two-level plan, and whatever a solve with many resumed blocks launches beyond stamp_cap.
	unsigned long long *stamps = nullptr;
	int n_stamps = 0, stamp_cap = 0;
	// what sweep_intervals read, kept for the next asker (a solve with many right-hand sides fills the stats of every result)
	mutable std::vector<std::pair<float, float>> sweep_iv;
	mutable int sweep_read = 0;       // 0: not read yet, 1: read, -1: read, and a slot or the copy was bad
};

// One solve: its plan, its side arrays and its resources.  Every resource has one owner, so a Solver is not copied: what starts
// from another one copies the SolverPlan, binds the ArenaPtrs and says what it borrows or acquires (make_view, factor_copy).
struct Solver : SolverPlan, ArenaPtrs, SolverHandles {
	SolverPlan &plan() { return *this; }
	const SolverPlan &plan() const { return *this; }
	Solver() = default;
	Solver(const Solver &) = delete;
	Solver &operator=(const Solver &) = delete;          // (another solve's plan: plan() = other.plan())
	~Solver() { release(); }
	// An owner gives everything back once its streams are idle; a view (make_view) what it acquired, and lets go of what it borrowed.
	void release()
	{
		if (!arena && !M && !tmp_src && !bs.held() && !sA && !sB && !ev0) return;     // nothing held
		(void)hipSetDevice(device);
		Pool &P = pool();
		bs.release(sA);
		if (view) {
			P.release_event(ev2, true);
			P.release_event(evx, true);
			arena = nullptr; M = nullptr; sA = sB = nullptr; ev0 = ev1 = ev3 = nullptr;          // (borrowed)
		} else {
			// nothing goes back to the pool while work may still be in flight (error paths return early)
			if (sC) (void)hipStreamSynchronize(sC);
			if (sB) (void)hipStreamSynchronize(sB);
			if (arena || M) (void)hipStreamSynchronize(sA);
			for (void *p : { arena, (void *)(ext_M ? nullptr : M), (void *)tmp_src, (void *)stamps }) P.release(p);
			for (hipEvent_t e : { ev0, ev1, ev2, ev3, evx }) P.release_event(e, true);
			for (hipEvent_t e : { evOuter, evPri, evPanelDone, evBig }) P.release_event(e, false);
			if (sC) P.release_stream(sC, device, nsys > 1 ? 3 : 1);
			for (hipEvent_t e : kev) P.release_event(e, true);
			for (hipEvent_t e : evA) P.release_event(e, false);
			for (hipEvent_t e : evPrio) P.release_event(e, false);
			if (own_sB && sB) P.release_stream(sB, device, nsys > 1 ? 3 : 1);
			if (own_sA && sA) P.release_stream(sA, device, false);
		}
		static_cast<ArenaPtrs &>(*this) = ArenaPtrs();
		static_cast<SolverHandles &>(*this) = SolverHandles();
	}
};

}  // namespace

struct gf2bv_result {
	int status = 0;
	i64 rank = 0, dim = 0, cw = 0;
	std::vector<u64> origin, basis;
	std::vector<int32_t> pivots;
	gf2bv_stats stats{};
};

namespace {

int check_device(int device)
{
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0)
		return fail(GF2BV_ERR_NODEVICE, "no HIP device visible: gf2bv_amd has no CPU fallback");
	if (device < 0 || device >= n) return fail(GF2BV_ERR_ARG, "device index out of range");
	HIPCHK(hipSetDevice(device));
	return GF2BV_OK;
}

// Two-level elimination: which blocks go in outer panels, and of how many blocks.
// An outer panel of K blocks saves HBM round trips -- the rows right of it make one trip per K blocks, and the outer pass runs
// 4.5-4.9 TB/s of sweep-words inside a solve (K = 8) where k_update16 runs 3.6-4.0 -- and costs ~0.4 ms of small launches per
// panel (k_outer_apply on two tile ranges, the priority part of the pass) plus a slower inner elimination beside the pass.
// Measured (K = 8 from the first block to the last full panel): 262144^2 1.517 -> 1.277 s, 131072^2 203 -> 195 ms, 98304^2 89 ->
// 100 ms, 65536^2 34 -> 47 ms; with a threshold on what remains right of the panel (profiles/r03_two_level.txt): 131072^2 best at
// 384-512 MiB (182 ms), 98304^2 at 512 MiB (87.3 against 92.8), 65536^2 never.  So: K = 8 while more than 512 MiB remain
// (262144^2: the first 75 % of the pivots; 131072^2: the first half; 98304^2: the first third; nothing below ~70000^2).
// GF2BV_TWO_LEVEL=0 turns it off, =K (2..12) forces K from the first block on for every full panel whatever the size (tests).
// Single systems on one GPU only: gangs and column-slab solves keep the one-level schedule.
void plan_two_level(Solver &S)
{
	S.tl_K = 0; S.tl_bend = 0; S.nsets = 2;
	// (a column-slab handle -- ext_M, at world size 1 too -- is driven block by block through slab_factor_on / slab_apply_on, which
	// know nothing of outer panels: with a plan it would skip the look-ahead at every panel end and never run an outer pass)
	if (S.world != 1 || S.ext_M || S.impl->G != GF2_GMAX) return;
	// gangs keep the one-level schedule.  Round 4 built outer panels for gangs (every outer kernel takes blockIdx.y = system) as an
	// opt-in, bit-exact and slower: 4.4 against 3.9 ms per system; round 5 measured it again on the final gang layout (a system per
	// XCD, streaming row accesses, gangs of 32 and of 8): 3.50-3.60 against 3.20-3.29 ms per system of 32768^2, K = 4 / 8 / 12 and
	// thresholds alike (profiles/r05_batch_scans.txt) -- a gang's inner elimination is a chain of all-rows launches of thousands of
	// workgroups that do not fit beside k_update16k, so chain and pass wait for each other instead of overlapping.  The opt-in
	// and its test are gone with round 5.
	if (S.nsys != 1) return;
	// outer panels of 12 blocks from 3 GiB up, of 8 below: the outer pass gains with K (isolated 5.20 / 5.30 / 5.38 TB/s of
	// sweep-words for K = 8 / 10 / 12), the inner elimination and the T chain grow with it -- 262144^2 1.303 -> 1.269 s,
	// 196608^2 566 -> 557 ms, 393216^2 4.26 -> 4.13 s, but 131072^2 184.0 -> 185.3 ms (profiles/r03_two_level.txt)
	int K = (double)S.rows * (double)S.wt * 8.0 >= 3.0 * 1073741824.0 ? GF2_KMAX : 8;       // (per system: a gang's panels stay at 8 blocks)
	double min_bytes = 0.5 * 1073741824.0;
	if (S.kn.two_level == 0) return;
	if (S.kn.two_level > 0) { K = S.kn.two_level; min_bytes = 0; }
	if (S.kn.two_level_min_set) min_bytes = 1048576.0 * S.kn.two_level_min_mib;      // (threshold scans)
	const int G = S.impl->G;
	int bend = 0;
	for (int b0 = 0; b0 + K < S.nblocks; b0 += K) {            // (the last block never ends an outer panel: it may be short)
		const i64 rows_left = S.rows - (i64)(b0 + K) * 64 * G, words_left = S.wt - (i64)(b0 + K) * G;
		if ((i64)(b0 + K) * 64 * G > S.cols || rows_left <= 0 || words_left <= 0) break;
		if ((double)rows_left * (double)words_left * 8.0 * (double)S.nsys < min_bytes) break;
		bend = b0 + K;
	}
	if (!bend) return;
	S.tl_K = K; S.tl_bend = bend;
	S.nsets = 2 * K;              // the outer pass of panel p reads its K sets while the blocks of panel p + 1 write theirs
}

int solver_alloc(Solver &S)
{
	const Knobs &kn = S.kn = Knobs::read();
	S.wt = (S.cols + S.nrhs + 63) / 64;
	S.cw = (S.cols + 63) / 64;
	S.npanels = (int)((S.cols + 63) / 64);
	S.maxr = std::min(S.rows, S.cols);
	S.impl = &kUpdates[S.kn.update];
	S.ntiles = tiles_for(S.wt);
	S.srows = slab_rows(S.rows);
	S.m_stride = S.ntiles * TW * S.srows;
	if (!S.M) HIPCHK(pool().alloc((void **)&S.M, sizeof(u64) * S.m_stride * S.nsys + kOuterSlackBytes, S.device));
	if (S.src && S.rows > 0) {
		k_to_tiled<<<dim3((unsigned)((S.rows + 63) / 64), (unsigned)((S.ntiles + 15) / 16), S.nsys), dim3(256), 0, S.sA>>>(
			S.src, S.stride, S.rows, S.ntiles, std::min(S.wt, S.stride), S.srows, S.M, S.src_sys_words, S.ss());
	}
	const int G = S.impl->G;
	S.nblocks = (S.npanels + G - 1) / G;
	S.tile_hi = S.ntiles;
	plan_two_level(S);
	S.units = (int)std::min<i64>(256, std::max<i64>(1, (S.rows + 255) / 256));
	// (a column-slab solve hands over through the host between the pieces: events; on one stream the panel gate would wait for a gate queued behind it)
	S.flag_sync = S.world == 1 && !kn.plain && kn.flag_sync != 0 && !kn.serial;
	S.optimistic = kn.optimistic >= 0 ? kn.optimistic != 0 : !kn.plain;
	S.xcd_pin = kn.xcd_pin >= 0 ? kn.xcd_pin != 0 : !kn.plain;
	if (kn.xcd_pin < 0 && !kn.plain && S.nsys >= 8 && S.nsys % 8 == 0) {           // a gang that would be pinned: is the dispatch order what the pinning assumes?
		int ok = 0;
		int rc = xcd_dispatch_is_round_robin(S.device, S.sA, &ok);
		if (rc) return rc;
		S.xcd_pin = ok != 0;
	}
	// narrow workgroups: as many rows each as keeps ~256 of them (all systems of a gang together) busy, at most 8 blocks
	{
		const i64 blocks = (S.rows + 255) / 256 * std::max(1, S.nsys);
		S.narrow_rpt = (int)std::min<i64>(8, std::max<i64>(1, blocks / 256));
	}
	if (kn.serial) { S.sB = S.sA; S.own_sB = false; }     // ablation: no look-ahead overlap
	else {
		// the bulk path yields to the (latency-critical) panel path wherever both have work queued: lowest priority
		// (round 5: single systems take a stream that is KNOWN to run beside sA, see Pool::low_stream_for.  Gangs take any: two
		// lock-step gangs side by side ran 16 MT19937 systems in 33 ms on whatever the pool handed out and in 36-41 ms on pairs
		// chosen this way -- with four busy queues other relations than panel / bulk of ONE solve decide, profiles/r05_stream_pairs.txt)
		if (S.nsys == 1) HIPCHK(pool().low_stream_for(kn, S.sA, S.device, &S.sB));
		else HIPCHK(pool().stream(&S.sB, S.device, 3));
		S.own_sB = true;
	}
	if (S.flag_sync && S.sB != S.sA) {
		int ok = 0;
		int rc = streams_run_concurrently(kn, S.device, S.sA, S.sB, &ok);
		if (rc) return rc;
		S.flag_sync = ok != 0;
	}
	// one arena for all side arrays (a dozen hipMalloc/hipFree pairs cost more than a small solve)
	{
		const ArenaLayout &L = S.lay = arena_layout(S);
		S.sync_base = 0;
		HIPCHK(pool().alloc(&S.arena, L.stride * S.nsys, S.device));
		S.bind(L, S.arena, kn.pc);
		// zero everything that is read before it is written: state, panel records, unit scratch, block bounds, multipliers
		for (int s = 0; s < S.nsys; s++) {
			char *b = (char *)S.arena + (size_t)s * L.stride;
			HIPCHK(hipMemsetAsync(b + L.st, 0, L.died - L.st, S.sA));
			HIPCHK(hipMemsetAsync(b + L.died, GF2_NEVER & 0xff, sizeof(int) * (size_t)std::max<i64>(1, S.rows), S.sA));
			HIPCHK(hipMemsetAsync(b + L.blk_first, 0, L.Wb - L.blk_first, S.sA));
		}
	}
	HIPCHK(pool().event(&S.ev0, true));
	HIPCHK(pool().event(&S.ev1, true));
	HIPCHK(pool().event(&S.ev2, true));
	HIPCHK(pool().event(&S.ev3, true));
	if (S.tl_K) {
		for (hipEvent_t *e : { &S.evOuter, &S.evPri, &S.evPanelDone }) HIPCHK(pool().event(e, false));
		if (S.sB != S.sA) { if (S.nsys == 1) HIPCHK(pool().low_stream_for(kn, S.sA, S.device, &S.sC)); else HIPCHK(pool().stream(&S.sC, S.device, 3)); }       // (GF2BV_SERIAL: everything on one stream)
		HIPCHK(pool().event(&S.evBig, false));
	}
	S.evA.resize(S.nblocks); S.evPrio.resize(S.nblocks); S.waitPrio.assign(S.nblocks, nullptr);
	for (int b = 0; b < S.nblocks; b++) {
		HIPCHK(pool().event(&S.evA[b], false));
		HIPCHK(pool().event(&S.evPrio[b], false));
	}
	return GF2BV_OK;
}

// Do kernels of two streams execute at the same time on this device, in this process?  (See k_probe_wait.)  Asked once per
// device; GF2BV_FLAG_SYNC=0 skips the question and the flag hand-over with it.
struct ConcurrencyCache { std::mutex mu; std::map<int, int> known; };
ConcurrencyCache &concurrency_cache() { static ConcurrencyCache c; return c; }
void forget_concurrency(int device)       // a gate timed out although the probe had passed: events from now on
{
	ConcurrencyCache &c = concurrency_cache();
	std::lock_guard<std::mutex> lk(c.mu);
	c.known[device] = 0;
}
int streams_run_concurrently(const Knobs &kn, int device, hipStream_t a, hipStream_t b, int *ok)
{
	std::mutex &mu = concurrency_cache().mu;
	std::map<int, int> &known = concurrency_cache().known;
	std::lock_guard<std::mutex> lk(mu);
	auto it = known.find(device);
	if (it != known.end()) { *ok = it->second; return GF2BV_OK; }
	if (kn.flag_sync == 2) { *ok = 1; return GF2BV_OK; }      // (taken for granted until a gate times out: exercises the time-out / retry path)
	int *d = nullptr;
	Held H(device, a); H.wait_for(b);
	HIPCHK(H.get((void **)&d, 2 * sizeof(int)));
	HIPCHK(hipMemsetAsync(d, 0, 2 * sizeof(int), a));
	HIPCHK(hipStreamSynchronize(a));
	HIPCHK(hipStreamSynchronize(b));
	k_probe_wait<<<dim3(1), dim3(1), 0, a>>>(d, d + 1, 200000ull);      // 2 ms
	k_probe_set<<<dim3(1), dim3(1), 0, b>>>(d);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(a));
	HIPCHK(hipStreamSynchronize(b));
	int h[2] = { 0, 0 };
	HIPCHK(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
	*ok = known[device] = (h[1] == 1);
	return GF2BV_OK;
}

// Does workgroup b of a one-dimensional launch sit on XCD b % 8 on this device?  The gang bulk update keeps a system's multipliers
// in ONE XCD's L2 on that assumption (speed only: results do not depend on it).  Asked once per device with k_probe_xcc -- 64
// workgroups report their XCC_ID: b and b + 8 must agree, 0..7 must differ.  Where it does not hold the gangs take the plain
// (spans, systems) grid of rounds 1-3.  GF2BV_XCD_PIN=1 / 0 skips the question.
int xcd_dispatch_is_round_robin(int device, hipStream_t st, int *ok)
{
	static std::mutex mu;
	static std::map<int, int> known;
	std::lock_guard<std::mutex> lk(mu);
	auto it = known.find(device);
	if (it != known.end()) { *ok = it->second; return GF2BV_OK; }
	int *d = nullptr;
	Held H(device, st);
	HIPCHK(H.get((void **)&d, 64 * sizeof(int)));
	int h[64];
	int good = 1;
	for (int rep = 0; rep < 2 && good; rep++) {          // (twice: the second launch starts where the first one left the dispatcher)
		k_probe_xcc<<<dim3(64), dim3(64), 0, st>>>(d);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		for (int b = 0; b < 64; b++) if (h[b] != h[b & 7]) good = 0;
		for (int a = 0; a < 8; a++) for (int b = a + 1; b < 8; b++) if (h[a] == h[b]) good = 0;
	}
	*ok = known[device] = good;
	return GF2BV_OK;
}

// Workgroups of one bulk-update launch (per system).  Each takes one contiguous span of the (tile, row)
// line (see k_update), so the count is free of the tile count: one workgroup per CU, fewer when a span
// would fall under ~4096 rows (a table build costs as much as streaming ~800 rows), shared among the
// systems of a gang.
int pick_update_wgs(i64 est_rows, int ntiles, int nsys, int pinned_wgs = 0)
{
	i64 want = 256;
	want = std::max<i64>(1, want / std::max(1, nsys));
	if (pinned_wgs > 0) want = pinned_wgs;          // XCD-pinned gangs: a system's workgroups fill ITS XCD (32 CUs), one system after the other
	// (a span below ~min_rows rows of a 64-byte column is not worth a workgroup of its own: a table build costs as much
	// as streaming ~1000 of them -- but small passes are latency, not throughput: the chip is mostly idle, so they take
	// as many workgroups as have at least that much to do)
	constexpr i64 min_rows = 2048;
	const i64 cap = std::max<i64>(1, (i64)ntiles * TW / 8 * est_rows / min_rows);
	return (int)std::min(want, cap);
}

// items (tiles, 4-word groups) in [first, end) that this rank owns -- units of 2^ulog items, see owned_item()
i64 owned_count(i64 first, i64 end, int ulog, int world, int wrank)
{
	if (end <= first) return 0;
	if (world <= 1) return end - first;
	i64 n = 0;
	for (i64 u = first >> ulog; u <= (end - 1) >> ulog; u++)
		if (u % world == wrank) n += std::min<i64>(end, (u + 1) << ulog) - std::max<i64>(first, u << ulog);
	return n;
}

// TRSM of block b on the 4-word groups [wlo / 4, end of the row) this rank owns
int launch_trsm(Solver &S, hipStream_t st, int j0, int gb, int wlo, int nw_lo, int nw_hi)
{
	constexpr int WPW = 4;
	const i64 g0 = wlo / WPW, g1 = S.tile_hi * TW / WPW;
	const i64 ng = owned_count(g0, g1, GF2_OWN_LOG - 2, S.world, S.wrank);
	if (ng <= 0) return GF2BV_OK;
	k_block_trsm<TW, WPW><<<dim3((unsigned)ng, S.nsys), dim3(64 * WPW), 0, st>>>(S.M, S.srows, j0, gb, wlo, (int)g0, S.world, S.wrank,
	                                                                           S.panels, S.aux, nw_lo, nw_hi, S.Pc, S.ss());
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// The stamp slot of the next timed launch: slot 0 is the clock at ev0, launch i takes slot i, and none is left (-1: that launch
// is bracketed by events) once `cap` are handed out.
constexpr int stamp_slot(int handed_out, int cap) { return handed_out >= 1 && handed_out < cap ? handed_out : -1; }
static_assert(stamp_slot(1, 66) == 1 && stamp_slot(65, 66) == 65, "slots 1 .. cap - 1 go to launches");
static_assert(stamp_slot(66, 66) == -1 && stamp_slot(67, 66) == -1, "a launch beyond the slots gets none: its last stamp would lie outside the buffer");
static_assert(stamp_slot(0, 66) == -1, "slot 0 is the base clock's");

// One bulk-update launch of block b on the `ntiles` owned tiles from tile_begin on; `last`: it carries the hand-off
// ("bulk of block b complete") and *handoff receives that event.
int launch_update_timed(Solver &S, hipStream_t st, int b, int j0, int gb, int wlo, u64 *mset, int tile_begin, int ntiles,
                        int nw_lo, bool last, hipEvent_t *handoff)
{
	// time_kernels: the launch stamps the clock itself; a launch beyond the slots (many resumed blocks) is bracketed by events
	hipEvent_t ka = nullptr, kb = nullptr;
	unsigned long long *t_first = nullptr, *t_last = nullptr;
	if (S.time_kernels && !S.stamps) return fail(GF2BV_ERR_HIP, "a timed bulk update without stamp slots (enqueue_forward_begin makes them)");
	if (const int slot = S.time_kernels ? stamp_slot(S.n_stamps, S.stamp_cap) : -1; slot > 0) {
		t_first = S.stamps + slot; t_last = t_first + S.stamp_cap;
		S.n_stamps++;
	} else if (S.time_kernels) {
		HIPCHK(pool().event(&ka, true)); HIPCHK(pool().event(&kb, true));
		S.kev.push_back(ka); S.kev.push_back(kb);
	}
	const i64 est_rows = std::max<i64>(256, S.rows - (i64)j0 * 64);      // alive rows of a dense system (the kernel uses the true bound)
	const bool pin = S.xcd_pin && S.nsys >= 8 && S.nsys % 8 == 0;
	const int wgs = pick_update_wgs(est_rows, ntiles, S.nsys, pin ? S.kn.xcd_wgs : 0);
	// the launch's own start / completion signals (hipExtLaunchKernel) carry the hand-off (or the timing events): no marker packets, ~1 % at every size
	const hipEvent_t begun = ka, done = kb ? kb : (last && !S.flag_sync ? S.evPrio[b] : nullptr);
	HIPCHK(S.impl->update(dim3((unsigned)wgs, S.nsys), st, S.M, S.rows, S.srows, j0, gb, wlo, S.panels, S.aux, mset,
	                      S.blk_first + b, tile_begin, ntiles, S.world, S.wrank, nw_lo, pin && S.kn.gang_nt,
	                      (const uint4 *)S.Pc, S.ss(), begun, done, pin ? S.nsys : 0, t_first, t_last));
	if (last && !S.flag_sync) *handoff = done;
	return GF2BV_OK;
}

// Forward elimination: all blocks, no host synchronisation.
//   stream A (panel path): factorise block b on its compact window (G+1 panel steps); then carry
//     block b+1's window forward (k_prio_window: block b's update on those <= 4 words of every row,
//     matrix -> Wb).  Needs the bulk update of block b-1 (stream B) to be complete, nothing newer.
//   stream B (bulk path): block b's TRSM + update on all trailing tiles, as soon as block b is
//     factorised, never writing the next window's words.  So A runs a whole block ahead of B and
//     the two overlap: per-block time is max(panel path, bulk path), and B never idles when it is
//     the longer one.
// ---- one block of the forward elimination, in the three pieces the two streams interleave ----
struct BlockGeom { int j0, gb, wlo, tb, nt_all, gnext; u64 *mset; };
BlockGeom block_geom(const Solver &S, int b)
{
	const int G = S.impl->G;
	BlockGeom g;
	g.j0 = b * G;
	g.gb = std::min(G, S.npanels - g.j0);
	g.wlo = g.j0 + g.gb;
	g.mset = S.mult + (i64)(b % S.nsets) * G * mult_rows(S.rows);
	// trailing tiles; the next block's window [wlo, wlo + gnext) sits in the first one or two of them
	// (two-level: the bulk kernels stop at the outer panel's end, and its last block has no next window to carry forward --
	// the outer pass covers that window like every other tile right of the panel)
	g.tb = g.wlo / TW;
	g.nt_all = (g.wlo < S.wt) ? (int)S.tile_hi - g.tb : 0;
	g.gnext = (b + 1 < S.nblocks && !S.ends_outer_panel(b)) ? std::min(G, S.npanels - g.wlo) : 0;
	return g;
}

bool fast_block_possible(const Solver &S, const BlockGeom &g)
{
	return S.kn.fast && g.gb == GF2_GMAX && (i64)(g.j0 + g.gb) * 64 <= S.cols && S.rows >= GF2_FAST_NC;
}

// Which way block b goes now.  A one-launch search alone only for a block that can take one at all, and never for the block that was
// just handed back; the dense one wants enough rows left, too.
BlockWay block_way(const Solver &S, int b)
{
	if (b == S.run.general_only || !fast_block_possible(S, block_geom(S, b))) return BlockWay::General;
	if (S.run.sparse_on) return BlockWay::SparseOnly;
	// rows left when the block starts: at most 64 leftover candidates sit below the bound besides the pivots found
	return S.run.dense_only && S.rows - (i64)b * 64 * S.impl->G >= GF2_FAST_NC + 128 ? BlockWay::DenseOnly : BlockWay::General;
}

// The pool sizes of k_block_sparse, by ForwardRun::tier (tests/sparse_cases.py: POOLS)
struct SparsePool { decltype(&k_block_sparse<256, 4>) search; int threads, rows; };
const SparsePool kSparsePools[] = {
	{ k_block_sparse<256, 4>, 256, 1024 },       // beside the bulk update
	{ k_block_sparse<512, 8>, 512, 4096 },       // after a give-up, or when the first block counted more rows than the small pool holds
	{ k_block_sparse<1024, 6>, 1024, 6144 },     // after two: 1024 threads at 128 registers, the candidates' words partly in scratch: slow, but still ahead of five general steps
};

// flag hand-over, panel stream: "block b factorised" (its multipliers are complete) -- and, where the look-ahead of block b
// follows (every block but the last), the wait for the bulk update of block b - 1 that k_prio_window needs
int panel_handover(Solver &S, int b)      // general panel steps: a launch for the announcement (k_narrow_all makes its own)
{
	k_gate<<<dim3(1, S.nsys), dim3(64), 0, S.sA>>>(S.sf, S.st, S.sync_base + b + 1, 0, 0, 0, S.ss());
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

constexpr int kSparseByDensity = 2;      // k_panel_step's search mode: it skips absent columns per chunk, by density (0 never, 1 always)
// stream A: factorise block b on its compact window -- step s narrows panel s-1 (window half (s-1)&1 -> half s&1)
// while searching panel s; gb+1 launches; evA[b] = "block b factorised"
int enqueue_block_panel(Solver &S, int b, BlockWay way = BlockWay::General)
{
	const BlockGeom g = block_geom(S, b);
	const unsigned row_blocks = (unsigned)((S.rows + 255) / 256);
	u64 *const half[2] = { S.Wb, S.Wb + (i64)GF2_GMAX * S.rows };
	// a one-launch block's last launch announces narrow_done itself (flag_sync) or carries evA[b] as its completion signal
	const hipEvent_t done = S.flag_sync ? nullptr : S.evA[b];
	const DoneSignal sig = S.flag_sync ? DoneSignal{ &S.sf->cnt_narrow, &S.sf->narrow_done, S.sync_base + b + 1 } : DoneSignal{};
	if (way == BlockWay::DenseOnly && S.kn.fused_narrow && S.nsys == 1) {
		// search + narrow step in one launch: workgroup 0 searches, the others narrow each panel as soon as it is formed
		// (single systems: a gang is throughput-bound, and its ~130 x nsys narrowing workgroups would hold their LDS for the whole
		// search -- measured equal either way, 243 against 242 systems/s of 32768^2: gangs keep the two launches)
		// at most ~128 narrowing workgroups: they stay resident for the whole search, and a CU that holds TWO of them (2 x 26 KiB
		// of LDS) cannot take a bulk-update workgroup (133 of 160 KiB) until they end -- with 257 workgroups on 256 CUs there is
		// always such a CU, and the pass whose launch lands just behind the search waits ~20 us for its last workgroup
		// (tools/pass_rates.py: every fourth pass of the mid-range of a 65536^2 solve)
		const int rpt = (int)std::min<i64>(8, std::max<i64>(S.narrow_rpt, (row_blocks + 127) / 128));
		hipExtLaunchKernelGGL(k_block_fast_narrow, dim3(1 + (row_blocks + rpt - 1) / rpt, S.nsys), dim3(256), 0, S.sA, nullptr, done, 0,
		                      S.M, S.rows, S.srows, g.j0, g.gb, b, (const u64 *)half[0], S.st, S.died, S.panels, S.aux, S.pivcol, S.urow,
		                      S.blk_first + b, S.Pfast, g.mset, S.impl->T, rpt, sig, S.ss());
		HIPCHK(hipGetLastError());
		return GF2BV_OK;
	}
	if (way == BlockWay::SparseOnly) {
		// sparse systems: the pool of the search = alive rows with a non-zero window (wmask, left by the look-ahead of the block before)
		const SparsePool &pool = kSparsePools[S.run.tier];
		pool.search<<<dim3(1, S.nsys), dim3(pool.threads), 0, S.sA>>>(S.M, S.rows, S.srows, g.j0, g.gb, 1, b, (const u64 *)half[0], S.st, S.died,
		                                                             S.panels, S.aux, S.pivcol, S.urow, S.blk_first + b, (const u64 *)S.wmask, S.ss());
	} else if (way == BlockWay::DenseOnly || fast_block_possible(S, g))
		// dense blocks: all G panels from a few hundred candidate rows in one launch; the general steps behind it find the
		// block done (or, when it gave up, untouched)
		k_block_fast<<<dim3(1, S.nsys), dim3(256), 0, S.sA>>>(S.M, S.rows, S.srows, g.j0, g.gb, way == BlockWay::DenseOnly, b, (const u64 *)half[0], S.st, S.died,
		                                                      S.panels, S.aux, S.pivcol, S.urow, S.blk_first + b, S.Pfast, S.ss());
	if (way != BlockWay::General) {
		hipExtLaunchKernelGGL(k_narrow_all, dim3((row_blocks + S.narrow_rpt - 1) / S.narrow_rpt, S.nsys), dim3(256), 0, S.sA, nullptr, done, 0,
		                      (const u64 *)S.M, S.rows, S.srows, g.j0, b, (const u64 *)half[0], (const SolveState *)S.st, (const int *)S.died,
		                      (const PanelAux *)S.aux, g.mset, S.impl->T, S.narrow_rpt, sig, S.ss());
		HIPCHK(hipGetLastError());
		return GF2BV_OK;
	}
	for (int s = 0; s <= g.gb; s++) {
		const int gp = s - 1, gf = (s < g.gb) ? s : -1;
		const i64 c0 = (i64)(g.j0 + std::max(gf, 0)) * 64;
		const u64 colmask = (S.cols - c0 >= 64) ? ~0ull : ((1ull << (S.cols - c0)) - 1);
		const int find_wgs = gf >= 0 ? (S.units + 3) / 4 : 0;
		const unsigned wgs = (unsigned)find_wgs + (gp >= 0 ? (row_blocks + S.narrow_rpt - 1) / S.narrow_rpt : 0u);
		// the block's last step carries the hand-off event as its own completion signal (no marker packet)
		const bool ext = !S.flag_sync && s == g.gb && b != S.nblocks - 1;
		hipExtLaunchKernelGGL(k_panel_step, dim3(wgs, S.nsys), dim3(256), 0, S.sA, nullptr, ext ? S.evA[b] : nullptr, 0,
		                      S.M, S.rows, S.srows, g.j0, gp, gf, g.gb, colmask,
		                      (const u64 *)half[s ? (s - 1) & 1 : 0], half[s & 1], S.st, S.died, S.fu, S.units, find_wgs,
		                      S.panels, S.aux, S.pivcol, S.urow, g.mset,
		                      gf == g.gb - 1 ? S.blk_first + b : (int *)nullptr, S.impl->T, kSparseByDensity, S.kn.self_wait_us * 100, S.narrow_rpt, b, S.ss());
	}
	if (b == S.nblocks - 1)
		k_win_scatter<<<dim3((unsigned)((S.rows * g.gb + 255) / 256), S.nsys), dim3(256), 0, S.sA>>>(S.M, S.rows, S.srows, g.j0, g.gb, half[g.gb & 1], S.died, S.st, S.ss());
	HIPCHK(hipGetLastError());
	if (S.flag_sync) { int rc = panel_handover(S, b); if (rc) return rc; }
	else if (b == S.nblocks - 1) HIPCHK(hipEventRecord(S.evA[b], S.sA));
	if (S.kn.debug_sync & 1) HIPCHK(hipDeviceSynchronize());
	return GF2BV_OK;
}

// stream B: TRSM + bulk update of block b on every trailing tile this rank owns (never WRITING the next window);
// waitPrio[b] = "bulk of block b complete"
int enqueue_block_bulk(Solver &S, int b)
{
	const BlockGeom g = block_geom(S, b);
	if (S.bulk_waits_outer) { HIPCHK(hipStreamWaitEvent(S.sB, S.evOuter, 0)); S.bulk_waits_outer = false; }
	if (S.flag_sync) {       // "bulk updates of the blocks before b complete"; wait for block b's multipliers
		// (submitted AFTER the launch that announces narrow_done and BEFORE the panel stream's gate that waits for bulk_done:
		// every wait targets earlier-submitted work.  A gate, not hipStreamWaitValue32: that is a polling kernel as well on this
		// runtime -- __amd_rocclr_streamOpsWait -- but one without a time-out)
		k_gate<<<dim3(1, S.nsys), dim3(64), 0, S.sB>>>(S.sf, S.st, 0, S.sync_base + b, S.sync_base + b + 1, 0, S.ss());
		HIPCHK(hipGetLastError());
	} else HIPCHK(hipStreamWaitEvent(S.sB, S.evA[b], 0));
	bool launched = false;
	if (g.nt_all > 0) {
		int rc = launch_trsm(S, S.sB, g.j0, g.gb, g.wlo, g.wlo, g.wlo + g.gnext);
		if (rc) return rc;
		// 16-byte tiles: the next block's window is whole tiles that are simply left out; when it ends in the middle of a
		// tile (an odd number of window words: the block before a short last one) that tile takes the HALF instance first
		// (the LAST block has no next window: its trailing words start at wlo, possibly in the middle of a tile whose first
		// word is the block's own -- the table entries are zero there, see `keep` in k_update16 -- and nobody else writes it)
		const int wend = g.wlo + g.gnext;
		const int tfull = g.gnext > 0 ? (wend + 1) / 2 : g.wlo / 2;      // first tile with no window word
		const i64 nfull = owned_count(tfull, S.tile_hi, GF2_OWN_LOG - 1, S.world, S.wrank);
		if ((wend & 1) && g.gnext > 0 && owned_count(wend / 2, wend / 2 + 1, GF2_OWN_LOG - 1, S.world, S.wrank) > 0) {
			rc = launch_update_timed(S, S.sB, b, g.j0, g.gb, g.wlo, g.mset, wend / 2, 1, -1, nfull <= 0, &S.waitPrio[b]);
			if (rc) return rc;
			launched = nfull <= 0;
		}
		if (nfull > 0) {
			rc = launch_update_timed(S, S.sB, b, g.j0, g.gb, g.wlo, g.mset, tfull, (int)nfull, 0, true, &S.waitPrio[b]);
			if (rc) return rc;
			launched = true;
		}
	}
	if (!launched && !S.flag_sync) {
		HIPCHK(hipEventRecord(S.evPrio[b], S.sB));      // "bulk of block b complete" (no update launch of this rank carries it)
		S.waitPrio[b] = S.evPrio[b];
	}
	if (S.kn.debug_sync & 2) HIPCHK(hipDeviceSynchronize());
	return GF2BV_OK;
}

// stream A: the next block's window (needs the bulk update of block b-1, nothing newer)
int enqueue_block_prio(Solver &S, int b)
{
	if (b + 1 >= S.nblocks || S.ends_outer_panel(b)) return GF2BV_OK;
	const BlockGeom g = block_geom(S, b);
	const unsigned row_blocks = (unsigned)((S.rows + 255) / 256);
	if (b > 0 && !S.flag_sync) HIPCHK(hipStreamWaitEvent(S.sA, S.waitPrio[b - 1], 0));
	// the bulk update of block b - 1: announced by the bulk stream's gate of block b (submitted before this one).  A k_gate
	// launch -- ONE spinning wavefront -- and not a wait inside k_prio_window (built in round 3: 32768^2 8.85 -> 8.7 ms): up
	// to thousands of workgroups spinning with 17 KiB of LDS each can sit on every CU before the bulk update they wait for
	// has been placed, which needs 133 KiB of a CU -- a deadlock until the time-out; seen at 327680^2 and beyond.
	if (b > 0 && S.flag_sync) {
		k_gate<<<dim3(1, S.nsys), dim3(64), 0, S.sA>>>(S.sf, S.st, 0, 0, 0, S.sync_base + b, S.ss());
		HIPCHK(hipGetLastError());
	}
	k_prio_window<<<dim3(row_blocks, S.nsys), dim3(256), 0, S.sA>>>(S.M, S.rows, S.srows, g.j0, g.gb, g.wlo, std::max(g.gnext, 1),
	                                                             S.panels, S.aux, g.mset, S.blk_first + b, S.Wb, S.Uwin,
	                                                             S.impl->T, S.st, S.ss(), (const int *)S.died, S.run.sparse_on ? S.wmask : (u64 *)nullptr);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

int enqueue_forward_begin(Solver &S, bool gather_first_window)
{
	if (S.time_kernels && !S.stamps) {
		// a slot per bulk-update launch: one per block, the HALF tile's, and room for blocks that are enqueued again
		S.stamp_cap = 2 * S.nblocks + 64;
		HIPCHK(pool().alloc((void **)&S.stamps, sizeof(unsigned long long) * 2 * S.stamp_cap, S.device));
		HIPCHK(hipMemsetAsync(S.stamps, 0xff, sizeof(unsigned long long) * S.stamp_cap, S.sA));                      // first: minima
		HIPCHK(hipMemsetAsync(S.stamps + S.stamp_cap, 0, sizeof(unsigned long long) * S.stamp_cap, S.sA));          // last: maxima
		k_stamp_clock<<<dim3(1), dim3(64), 0, S.sA>>>(S.stamps);
		HIPCHK(hipGetLastError());
		S.n_stamps = 1;
	}
	HIPCHK(hipEventRecord(S.ev0, S.sA));
	HIPCHK(hipStreamWaitEvent(S.sB, S.ev0, 0));     // sB starts after the setup memsets on sA
	if (S.npanels > 0 && gather_first_window) {
		const int g0 = std::min(S.impl->G, S.npanels);
		k_win_gather<<<dim3((unsigned)((S.rows * g0 + 255) / 256), S.nsys), dim3(256), 0, S.sA>>>(S.M, S.rows, S.srows, 0, g0, S.Wb, S.st, S.ss());
	}
	return GF2BV_OK;
}

// join: the panel stream waits for the last bulk update; pivot rows get their parked window words
int enqueue_forward_join(Solver &S)
{
	HIPCHK(hipEventRecord(S.ev3, S.sB));
	HIPCHK(hipStreamWaitEvent(S.sA, S.ev3, 0));
	if (S.nblocks > 1 && S.maxr > 0)
		k_unwind<<<dim3((unsigned)((S.maxr * GF2_GMAX + 255) / 256), S.nsys), dim3(256), 0, S.sA>>>(
			S.M, S.srows, S.impl->G, S.npanels, S.nblocks, S.st, S.pivcol, S.urow, S.Uwin, S.world, S.wrank, S.tl_K, S.tl_bend, S.ss());
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

int enqueue_check_rhs(Solver &S)
{
	int g = (int)std::min<i64>(1024, (S.rows + 255) / 256);
	if (S.rhs_bad) {
		const i64 nrw = ((S.cols & 63) + S.nrhs + 63) / 64;
		k_check_rhs_many<<<dim3(g, (unsigned)std::min<i64>(nrw, 65535)), dim3(256), 0, S.sA>>>(S.M, S.rows, S.srows, S.cols, S.nrhs,
		                                                                                      S.died, S.rhs_bad);
	} else {
		k_check_rhs<<<dim3(g, S.nsys), dim3(256), 0, S.sA>>>(S.M, S.rows, S.srows, S.cols, S.died, S.st, S.ss());
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(S.ev1, S.sA));
	return GF2BV_OK;
}

// Two-level elimination: the row lists and T of the panel that starts at block b0 -- two buffers of each, by panel parity (the
// previous panel's outer pass may still be reading its own)
struct OuterBufs { int *prow; u64 *Tm; };
OuterBufs outer_bufs(const Solver &S, int b0)
{
	const size_t parity = (size_t)((b0 / S.tl_K) % S.nlist);
	return { S.oprow + parity * GF2_OUTER_LISTS, S.Tm + parity * ((size_t)GF2_KMAX * GF2_KMAX * GF2_GMAX * 64 * GF2_GMAX) };
}

// Two-level elimination, the outer step of the panel of blocks [b0, b1) on the column tiles [t_begin, t_end): pivot rows
// brought up to date there (k_outer_trsm), then all the panel's blocks applied in one pass (k_update16k).  One workgroup per
// ITEM (tile, chunk of rows) -- not persistent ones: CUs come free all the time, and the next panel's elimination, whose
// streams rank above this one, slips its kernels in between (a persistent launch filled every CU until its very end: the
// look-ahead had nowhere to run; reserving CUs for it cost the pass more than the overlap gave back).
// What the outer step of the panel of blocks [b0, b1) needs from its records alone: the row lists and T (P = T x S: the chain
// of panel steps run ONCE, on the identity, one workgroup per source block).  Enqueued on the PANEL stream right behind the
// panel's last block: it runs while the outer stream is still busy with the previous panel's pass (0.26 ms off its path).
int enqueue_outer_prepare(Solver &S, hipStream_t st, int b0, int b1)
{
	const int G = S.impl->G;
	const i64 set_words = (i64)G * mult_rows(S.rows);
	const int npan = (b1 - b0) * G;
	const OuterBufs ob = outer_bufs(S, b0);
	k_outer_prow<<<dim3(1, S.nsys), dim3(256), 0, st>>>(b0 * G, b1 - b0, S.panels, S.aux, ob.prow, S.ss());
	if (!S.kn.outer_chain)
		k_outer_trsm<4, true><<<dim3((unsigned)(npan / 4), S.nsys), dim3(256), 0, st>>>(S.M, S.rows, S.srows, b0 * G, npan, 0, S.panels, S.aux, S.mult,
		                                                                               set_words, b0 % S.nsets, S.nsets, S.impl->T, ob.Tm, S.ss());
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// The outer step of the panel of blocks [b0, b1) on the tiles [t_begin, t_end): the panel's pivot rows P = T x S there (k_outer_apply;
// GF2BV_OUTER_CHAIN=1: the chain itself on every word group), then the pass (k_update16k_wide, one workgroup per item, chunk-major).
int enqueue_outer_apply(Solver &S, hipStream_t st, int b0, int b1, i64 t_begin, i64 t_end)
{
	const int G = S.impl->G;
	const i64 nt = t_end - t_begin;
	if (nt <= 0) return GF2BV_OK;
	const i64 set_words = (i64)G * mult_rows(S.rows);
	const OuterBufs ob = outer_bufs(S, b0);
	const int npan = (b1 - b0) * G;
	if (S.kn.outer_chain) {
		const i64 g_begin = t_begin * TW / 4, ng = t_end * TW / 4 - g_begin;
		k_outer_trsm<4, false><<<dim3((unsigned)ng, S.nsys), dim3(256), 0, st>>>(S.M, S.rows, S.srows, b0 * G, npan, (int)g_begin, S.panels, S.aux,
		                                                                          S.mult, set_words, b0 % S.nsets, S.nsets, S.impl->T, (u64 *)nullptr, S.ss());
	} else
		k_outer_apply<<<dim3((unsigned)nt, S.nsys), dim3(512), 0, st>>>(S.M, S.rows, S.srows, b1 - b0, (const int *)ob.prow, (const u64 *)ob.Tm, (int)t_begin, S.ss());
	HIPCHK(hipGetLastError());
	hipEvent_t ka = nullptr, kb = nullptr;
	if (S.time_kernels) {
		HIPCHK(pool().event(&ka, true)); HIPCHK(pool().event(&kb, true));
		S.kev.push_back(ka); S.kev.push_back(kb);
	}
	// items of a dense system: the kernel derives the true count from the alive bound and loops if there are more
	const i64 est_lo = std::min<i64>(S.rows, (i64)b0 * 64 * G) & ~(i64)63, R64 = round_up(S.rows, 64);
	constexpr i64 item_rows = (i64)GF2_WSEG * 1024;
	static_assert((size_t)item_rows * 32 <= kOuterSlackBytes, "the slack behind the matrix covers an item");
	const i64 nch = std::max<i64>(1, (R64 - est_lo + item_rows - 1) / item_rows);
	const i64 wgs = std::min<i64>(nch * nt, (i64)1 << 30);
	hipExtLaunchKernelGGL(k_update16k_wide, dim3((unsigned)wgs, S.nsys), dim3(1024), 0, st, ka, kb, 0,
	                      S.M, S.rows, S.srows, b1 - b0, (const int *)ob.prow, (const u64 *)S.mult,
	                      set_words, b0 % S.nsets, S.nsets, (const int *)(S.blk_first + b0), (const int *)S.died, b1 * G, (int)t_begin, (int)nt, S.ss(), 1);
	HIPCHK(hipGetLastError());
	if (S.kn.debug_sync & 2) HIPCHK(hipDeviceSynchronize());
	return GF2BV_OK;
}

int enqueue_window_gather(Solver &S, int b)
{
	const BlockGeom g = block_geom(S, b);
	k_win_gather<<<dim3((unsigned)((S.rows * g.gb + 255) / 256), S.nsys), dim3(256), 0, S.sA>>>(S.M, S.rows, S.srows, g.j0, g.gb, S.Wb, S.st, S.ss());
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// The solve's state as the panel stream has left it, on the host (a host wait: everything submitted to the panel stream has run)
int read_state(Solver &S, SolveState *hst)
{
	HIPCHK(hipMemcpyAsync(hst, S.st, sizeof *hst, hipMemcpyDeviceToHost, S.sA));
	HIPCHK(hipStreamSynchronize(S.sA));
	return GF2BV_OK;
}

// A one-launch search could not take block pb and poisoned the panel path from there on (SolveState::poison, read by the host): every
// later panel-path kernel has returned at once, the bulk and outer kernels found no pivots for the unpublished blocks and did nothing,
// and the matrix and the window buffer are exactly as that block needs.  Everything in flight is drained, the plan cut back to what
// has run and the counters rebased; block pb takes the general steps when the caller enqueues it again, and the blocks behind it the
// next pool size -- or, where the host looked at the block before anything was enqueued behind it (`rearm`), the largest at once if the
// search counted more rows than the middle pool holds (`want`); a hand-back met after submission knows no `want` and takes no further
// look.  Give-ups of the sparse search are counted, by the kernel's reason too; the third of a solve switches it off.
int hand_back(Solver &S, int pb, const SolveState &hst, int want, bool rearm)
{
	if (S.sC) HIPCHK(hipStreamSynchronize(S.sC));
	HIPCHK(hipStreamSynchronize(S.sB));
	// (two-level: the outer panels before the poisoned one are complete; the published blocks of the poisoned panel have been
	// applied to its own tiles by the bulk kernels and to everything right of it by its outer pass -- every tile has seen
	// exactly the blocks before pb -- so the rest runs as a one-level schedule)
	if (S.tl_K && pb < S.tl_bend) S.tl_bend = pb / S.tl_K * S.tl_K;
	S.bulk_waits_outer = false;
	HIPCHK(hipMemsetAsync(&S.st->poison, 0, sizeof(int), S.sA));
	S.sync_base += S.nblocks + 1;
	ForwardRun &run = S.run;
	run.dense_only = false;
	if (run.sparse_on) {
		if (hst.sp_why >= 1 && hst.sp_why <= 5) run.why[hst.sp_why - 1]++;
		if (++run.giveups >= 3) run.sparse_on = false;
		if (rearm && run.sparse_on) run.probes = 1;      // (the larger pools get one look each, too)
	}
	static_assert(sizeof kSparsePools == 3 * sizeof kSparsePools[0], "ForwardRun::tier indexes kSparsePools; gf2bv_stats::sparse_blocks[3] counts by it");
	run.tier = std::min(2, std::max(run.tier + 1, want));
	run.general_only = pb;
	return GF2BV_OK;
}

// One block of the forward pass: panel path, bulk path, the next block's window.
// Sparse systems (round 5): when block 0 did NOT take the dense search, the following full blocks get k_block_sparse + k_narrow_all
// instead of the G + 1 general panel steps (one-level schedules only; the look-ahead of every block leaves the masks the next
// block's pool is taken from).  A block it cannot take is handed back like a failed optimistic block: THAT block takes the general
// steps and the search goes on behind it -- twice; the third give-up of a solve switches it off and the rest runs general.
int forward_block(Solver &S, int blk)
{
	int rc;
	SolveState hst;
	const BlockWay way = block_way(S, blk);
	if ((rc = enqueue_block_panel(S, blk, way))) return rc;
	if (way == BlockWay::SparseOnly && S.run.probes > 0) {
		S.run.probes--;
		if ((rc = read_state(S, &hst))) return rc;
		// the pool for the blocks behind this one: a search that counted far more rows with a bit in its window than the middle pool
		// holds goes straight to the largest (MT19937, one bit per output: 4500-5000).  Otherwise the SMALL pool stays while it works,
		// truncated or not -- it is the one that fits beside the bulk update, and the first 1024 candidate rows usually hold a panel's
		// pivots (measured: 17 / 1337 / 137 bits per output count 1100-1560 rows and run 7.4 / 6.3 / 6.7 ms on the small pool, 7.9 /
		// 7.1 / 7.4 on the middle one); a pool that does not gives up and the next size takes over
		const int want = hst.sp_nz > 3400 ? 2 : 0;
		if (hst.poison) return (rc = hand_back(S, blk, hst, want, true)) ? rc : forward_block(S, blk);      // (the same block again: general)
		S.run.tier = std::max(S.run.tier, want);
	}
	if ((rc = enqueue_block_bulk(S, blk))) return rc;
	if ((rc = enqueue_block_prio(S, blk))) return rc;
	// Optimistic enqueue for dense systems.  k_block_fast decides ON THE DEVICE whether a block goes the fast way, so the
	// general panel steps have to be enqueued behind it all the same, and on a fast block they are G + 1 empty launches
	// of ~4.5 us each on the critical path (and, beside an outer pass, ~500 workgroups each that take CUs from it).  One look
	// at the device settles it for the usual case: block 0 is enqueued both ways and the host waits for its panel path (a
	// ~50 us stall, once per solve); if the fast search took it, the blocks that can take it at all (full blocks with enough
	// rows left) get k_block_fast + k_narrow_all only.  Should the search give up on one of them after all, the host resumes
	// from that block (hand_back) with both paths and the one-level schedule.
	if (blk == 0 && S.kn.fast && S.optimistic && S.nsys == 1 && S.world == 1 && S.nblocks >= 8 && fast_block_possible(S, block_geom(S, 0))) {
		if ((rc = read_state(S, &hst))) return rc;
		S.run.dense_only = hst.fast_done == 1;
		if (!S.run.dense_only && S.kn.sparse_fast && S.tl_K == 0 && S.nblocks > 1) {
			// block 1's window is in place (the look-ahead above ran without masks): its masks by a launch of their own
			S.run.sparse_on = true;
			k_window_masks<<<dim3((unsigned)((S.rows + 255) / 256), S.nsys), dim3(256), 0, S.sA>>>((const u64 *)S.Wb, S.rows, block_geom(S, 1).gb, (const int *)S.died,
			                                                                                      S.wmask, (const SolveState *)S.st, S.ss());
			HIPCHK(hipGetLastError());
		}
	}
	return GF2BV_OK;
}

// Two-level part (large single systems, plan_two_level): outer panels of tl_K blocks.  Inside a panel the blocks run
// exactly as in the one-level loop -- panel and bulk stream, look-ahead from block to block -- with the bulk kernels
// confined to the panel's own tiles (tile_hi).  The outer step of panel p goes to a THIRD stream in two parts: first the
// tiles of panel p + 1 (a small launch), behind which that panel's first window is gathered and its elimination starts,
// then everything right of them, one workgroup per item so that the next panel's kernels find CUs while it runs.  What
// the two meet in: the multiplier sets (2 K of them: panel parity), the pivot marks (k_update16k takes "alive behind
// panel p", not "alive now") and disjoint tiles.  Leaves the window of block tl_bend, the first of the one-level part, in place.
int enqueue_outer_panels(Solver &S)
{
	int rc;
	const int G = S.impl->G;
	hipStream_t so = S.sC ? S.sC : S.sB;           // (GF2BV_SERIAL: one stream, everything in order)
	bool big_recorded = false;                     // evBig holds the end of the previous panel's pass (side launches)
	for (int p0 = 0; p0 < S.tl_bend; p0 += S.tl_K) {
		const int p1 = p0 + S.tl_K;
		if (p0 > 0) {
			HIPCHK(hipStreamWaitEvent(S.sA, S.evPri, 0));
			if ((rc = enqueue_window_gather(S, p0))) return rc;
		}
		S.tile_hi = (i64)p1 * G / TW;
		for (int b = p0; b < p1; b++)
			if ((rc = forward_block(S, b))) return rc;
		S.tile_hi = S.ntiles;
		// the outer step needs the panel's records and multipliers (panel stream), not its bulk updates (other tiles)
		if ((rc = enqueue_outer_prepare(S, S.sA, p0, p1))) return rc;
		HIPCHK(hipEventRecord(S.evPanelDone, S.sA));
		HIPCHK(hipStreamWaitEvent(so, S.evPanelDone, 0));
		const i64 t0 = (i64)p1 * G / TW, t1 = std::min<i64>(S.ntiles, t0 + (i64)S.tl_K * G / TW);
		// (late round 5) the outer step on the NEXT panel's tiles -- a short launch on an underused chip, ~0.3 ms -- goes to the
		// inner elimination's bulk stream, idle at this point, and runs BESIDE the start of the pass proper instead of before it:
		// it needs the previous pass complete (evBig; it used to follow it in stream order) and this panel's T; the pass proper
		// needs T alone (disjoint tiles).  No new stream.
		hipStream_t sn = S.kn.outer_side && S.sB != so && S.sB != S.sA ? S.sB : so;
		if (sn != so) {
			HIPCHK(hipStreamWaitEvent(sn, S.evPanelDone, 0));
			if (big_recorded) HIPCHK(hipStreamWaitEvent(sn, S.evBig, 0));
		}
		if ((rc = enqueue_outer_apply(S, sn, p0, p1, t0, t1))) return rc;
		HIPCHK(hipEventRecord(S.evPri, sn));
		if ((rc = enqueue_outer_apply(S, so, p0, p1, t1, S.ntiles))) return rc;
		// (round 6, VERDICT item 2a: P = T x S of the NEXT panel started behind the first chunk of this pass, beside its rest -- built,
		// bit-exact, no gain: the launch is LDS table work like the pass itself, not idle chip time.  profiles/r06_outer_early.txt)
		HIPCHK(hipEventRecord(S.evBig, so));
		big_recorded = true;
	}
	HIPCHK(hipEventRecord(S.evOuter, so));
	HIPCHK(hipStreamWaitEvent(S.sA, S.evPri, 0));
	if (S.tl_bend < S.nblocks && (rc = enqueue_window_gather(S, S.tl_bend))) return rc;
	S.bulk_waits_outer = S.sC != nullptr;          // the one-level bulk updates behind it touch every trailing tile
	return GF2BV_OK;
}

int enqueue_forward(Solver &S)
{
	Trace tr;
	int rc = enqueue_forward_begin(S, true);
	if (rc) return rc;
	if (S.tl_K && (rc = enqueue_outer_panels(S))) return rc;
	for (int b = S.tl_K ? S.tl_bend : 0; b < S.nblocks; b++)
		if ((rc = forward_block(S, b))) return rc;
	if ((rc = enqueue_forward_join(S))) return rc;
	tr.mark(S.kn, "forward: all blocks submitted");          // (host side only: the device is still working; what follows waits for it)
	// everything is submitted: a block a search handed back shows only now -- resume there, join again, look again
	while (S.run.dense_only || S.run.sparse_on) {
		SolveState hst;
		if ((rc = read_state(S, &hst))) return rc;
		if (!hst.poison) break;
		const int pb = hst.poison - 1;
		if ((rc = hand_back(S, pb, hst, 0, false))) return rc;
		// (the poisoned block's window is in place; the blocks behind it take their masks from the look-aheads again)
		for (int b = pb; b < S.nblocks; b++)
			if ((rc = forward_block(S, b))) return rc;
		if ((rc = enqueue_forward_join(S))) return rc;
	}
	return enqueue_check_rhs(S);
}

// The one way into a back-substitution of the columns `cols` on S (each of its nsys systems): what an earlier one on this Solver
// still holds goes back first; then the columns are kept and uploaded, and the solutions are cleared.  Every buffer is S.bs's from
// the moment it exists, so a failure part-way leaves nothing that the next begin or the Solver's release does not return.
int backsub_begin(Solver &S, const std::vector<int> &cols)
{
	BackSub &B = S.bs;
	B.release(S.sA);
	B.cols = cols;
	B.ny = (int)cols.size();
	const size_t out_bytes = sizeof(u64) * B.ny * std::max<i64>(1, S.cw) * S.nsys;
	HIPCHK(pool().alloc((void **)&B.ycols, sizeof(int) * B.ny, S.device));
	HIPCHK(hipMemcpyAsync(B.ycols, B.cols.data(), sizeof(int) * B.ny, hipMemcpyHostToDevice, S.sA));
	HIPCHK(pool().alloc((void **)&B.out, out_bytes, S.device));
	HIPCHK(hipMemsetAsync(B.out, 0, out_bytes, S.sA));
	return GF2BV_OK;
}

// back-substitution on Y = selected columns of U (RHS [+ free columns]); then scatter.
int enqueue_backward(Solver &S, const std::vector<int> &cols)
{
	int rc = backsub_begin(S, cols);
	if (rc) return rc;
	BackSub &B = S.bs;
	const i64 nyw = (B.ny + 63) / 64;
	B.ys = round_up(nyw, YTW);
	HIPCHK(pool().alloc((void **)&B.Y, sizeof(u64) * std::max<i64>(1, S.maxr) * B.ys, S.device));
	HIPCHK(hipMemsetAsync(B.Y, 0, sizeof(u64) * std::max<i64>(1, S.maxr) * B.ys, S.sA));
	u64 *bmult = S.mult;              // forward multipliers are dead by now
	const int rpb = 2048;
	if (S.maxr > 0) {
		// (a launch dimension holds fewer than 2^32 work-items: pivots go in chunks of 2^24 wavefronts)
		const i64 kchunk = std::max<i64>(1, (1ll << 24) / nyw);
		for (i64 k0 = 0; k0 < S.maxr; k0 += kchunk) {
			const i64 waves = std::min(kchunk, S.maxr - k0) * nyw;
			k_extract_y<<<dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, S.sA>>>(S.M, S.srows, S.st, S.urow, S.pivcol,
			                                                                      B.ycols, B.ny, B.Y, B.ys, k0);
		}
		const int ytiles = (int)(B.ys / YTW);
		for (int q = S.npanels - 1; q >= 1; q--) {
			const i64 bound = std::min<i64>((i64)64 * q, S.maxr);      // pivots before panel q
			int g = (int)std::min<i64>(1024, (bound + 255) / 256);
			k_gather_mult_u<<<dim3(g), dim3(256), 0, S.sA>>>(S.M, S.srows, q, S.panels + q, S.urow, bmult);
			const i64 nrb = (bound + rpb - 1) / rpb;
			HIPCHK(launch_ysweep(dim3((unsigned)(ytiles * nrb)), S.sA, B.Y, B.ys, S.maxr, S.panels + q, bmult, ytiles, rpb));
		}
		for (i64 k0 = 0; k0 < S.maxr; k0 += kchunk << 6) {
			const i64 thr = std::min(kchunk << 6, S.maxr - k0) * nyw;
			k_scatter_solution<<<dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, S.sA>>>(B.Y, B.ys, S.st, S.pivcol, B.ny,
			                                                                              B.out, std::max<i64>(1, S.cw), k0);
		}
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(S.ev2, S.sA));
	return GF2BV_OK;
}

// Blocked parity back-substitution straight into the solution words (no Y matrix), for up to GF2_BSV
// right-hand sides at once: solve_one (the RHS column) and small kernel bases (the free columns + RHS).
// U is streamed once for all of them.
// A gang (S.nsys > 1) runs the same chain once for all its systems, blockIdx.y = system -- 2 x ceil(npanels / 16) launches for the
// gang instead of as many per system (a 32768^2 system's chain is 64 launches of 6 + 13 us: 1.2 ms during which one workgroup
// walks a diagonal block; 24 of them in a row were 15 % of a gang's wall time, profiles/r04_batch_budget.txt).  The gang owns the
// buffers, system s finds its solution at out + s * cw (BackSub::borrow).  One column per system then, and no inverted blocks:
// k_bs_near2 takes no system stride.
int enqueue_backward_parity(Solver &S, const std::vector<int> &cols)
{
	if (S.nsys > 1 && cols.size() != 1) return fail(GF2BV_ERR_ARG, "a gang's back-substitution solves for one column per system");
	int rc = backsub_begin(S, cols);
	if (rc) return rc;
	BackSub &B = S.bs;
	const i64 cw = std::max<i64>(1, S.cw);
	const unsigned nsys = (unsigned)S.nsys;
	unsigned char *accv = reinterpret_cast<unsigned char *>(S.mult);     // forward multipliers are dead by now (2*G*8 bytes per row)
	const i64 nacc = std::max<i64>(1, S.maxr);
	// the diagonal blocks of U, gathered by the whole chip into compact form for the serial walk of k_bs_near
	const i64 dgw = (i64)64 * 16 * std::max(1, S.npanels);
	HIPCHK(pool().alloc((void **)&B.Y, sizeof(u64) * dgw * nsys, S.device));
	if (S.npanels > 0)
		k_bs_diag<<<dim3(S.npanels, nsys), dim3(256), 0, S.sA>>>(S.M, S.srows, S.npanels, S.panels, S.urow, B.Y, S.ss(), dgw);
	// Round 4: from sixteen groups (16384 columns) up the diagonal blocks are inverted up front (k_bs_inv, all groups in one launch, ~90 us) and the
	// serial walk of a link (k_bs_near, 12 us) becomes a matrix-vector product (k_bs_near2, ~4 us).  GF2BV_BS_INV=0 / 1: never / always.
	const int ngroups = (S.npanels + GF2_BSG - 1) / GF2_BSG;
	const bool inv = nsys == 1 && (S.kn.bs_inv >= 0 ? S.kn.bs_inv != 0 && ngroups >= 1 : ngroups >= 16);
	if (inv) {
		HIPCHK(pool().alloc((void **)&B.Minv, sizeof(u64) * (size_t)ngroups * 16 * 64 * 16, S.device));
		static std::mutex mu;
		static std::map<int, bool> raised;          // device -> the > 64 KiB dynamic-LDS attribute has been raised there
		{
			std::lock_guard<std::mutex> lk(mu);
			if (!raised[S.device]) {
				HIPCHK(hipFuncSetAttribute((const void *)k_bs_inv, hipFuncAttributeMaxDynamicSharedMemorySize, GF2_BSINV_LDS));
				raised[S.device] = true;
			}
		}
		k_bs_inv<<<dim3(ngroups), dim3(1024), GF2_BSINV_LDS, S.sA>>>(B.Y, S.npanels, S.panels, S.pivcol, B.Minv);
	}
	// right-hand sides in groups of GF2_BSV (U is streamed once per group; the groups are independent)
	for (int v0 = 0; v0 < B.ny; v0 += GF2_BSV) {
		const int nv = std::min(GF2_BSV, B.ny - v0);
		u64 *X = B.out + (i64)v0 * cw;
		for (int qb = S.npanels; qb > 0; qb -= GF2_BSG) {
			const int qa = std::max(0, qb - GF2_BSG);
			const int waves = (qb - qa) * 64;
			k_bs_far<<<dim3((waves + 3) / 4, nsys), dim3(256), 0, S.sA>>>(S.M, S.srows, cw, qa, qb, S.panels, S.urow, S.pivcol, B.ycols + v0, nv,
			                                                              X, accv, nacc, S.ss(), cw);
			if (inv)
				k_bs_near2<<<dim3(1), dim3(1024), 0, S.sA>>>(cw, qa, qb, S.panels, S.pivcol, nv, X, accv, nacc, B.Minv, (S.npanels - qb) / GF2_BSG);
			else
				k_bs_near<<<dim3(1, nsys), dim3(256), 0, S.sA>>>(B.Y, cw, qa, qb, S.panels, S.pivcol, nv, X, accv, nacc, S.ss(), dgw, cw);
		}
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(S.ev2, S.sA));
	return GF2BV_OK;
}

// Back-substitution of the columns cols: up to GF2_BS_MAXRHS of them (kernel dimensions of the reference's use: solve_all
// caps at 16) the parity path, GF2_BSV of them per pass over U; more: the table sweeps over the bit matrix Y (one pass over Y
// per panel whatever the dimension).  GF2BV_YSWEEP sends every count to the sweeps (the general path, for cross-checking).
int enqueue_backsub(Solver &S, const std::vector<int> &cols)
{
	if ((i64)cols.size() <= GF2_BS_MAXRHS && !S.kn.ysweep) return enqueue_backward_parity(S, cols);
	return enqueue_backward(S, cols);
}

int solver_enqueue(Solver &S)
{
	Trace tr;
	int rc = solver_alloc(S);
	tr.mark(S.kn, "solver_alloc");
	if (rc) return rc;
	rc = enqueue_forward(S);
	tr.mark(S.kn, "enqueue_forward");
	if (rc) return rc;
	if (S.mode == GF2BV_MODE_SINGLE) return enqueue_backsub(S, { (int)S.cols });
	return GF2BV_OK;
}

// The free columns in M4RI's kernel order (_internal.c:348): positions rank .. cols of the identity
// permutation after position i was swapped with piv[i], i < rank, in turn
std::vector<int> m4ri_free_order(const int32_t *piv, i64 rank, i64 cols)
{
	std::vector<int> order(cols);
	for (i64 i = 0; i < cols; i++) order[i] = (int)i;
	for (i64 i = 0; i < rank; i++) std::swap(order[i], order[piv[i]]);
	return std::vector<int>(order.begin() + rank, order.end());
}

// The kernel basis needs rank and pivot columns on the host (one sync) to lay out the free columns in M4RI's order:
// S.hst and S.free_order.
int load_free_order(Solver &S)
{
	HIPCHK(hipMemcpyAsync(&S.hst, S.st, sizeof S.hst, hipMemcpyDeviceToHost, S.sA));
	HIPCHK(hipStreamSynchronize(S.sA));
	std::vector<int32_t> piv(S.hst.rank);
	if (S.hst.rank)
		HIPCHK(hipMemcpy(piv.data(), S.pivcol, sizeof(int) * S.hst.rank, hipMemcpyDeviceToHost));
	S.free_order = m4ri_free_order(piv.data(), S.hst.rank, S.cols);
	return GF2BV_OK;
}

// The asynchronous device-to-host copies of everything a result needs (state, back-substitution output, panel records,
// pivot columns), then S.evx.
int enqueue_export(Solver &S)
{
	if (!S.evx) HIPCHK(pool().event(&S.evx, true));
	HIPCHK(hipMemcpyAsync(&S.hst, S.st, sizeof S.hst, hipMemcpyDeviceToHost, S.sA));
	S.hout.resize((size_t)S.bs.ny * std::max<i64>(1, S.cw));
	HIPCHK(hipMemcpyAsync(S.hout.data(), S.bs.out, sizeof(u64) * S.hout.size(), hipMemcpyDeviceToHost, S.sA));
	S.hp.resize(std::max(1, S.npanels));
	HIPCHK(hipMemcpyAsync(S.hp.data(), S.panels, sizeof(PanelRec) * S.hp.size(), hipMemcpyDeviceToHost, S.sA));
	S.hpiv.resize(std::max<i64>(1, S.maxr));
	HIPCHK(hipMemcpyAsync(S.hpiv.data(), S.pivcol, sizeof(int) * S.hpiv.size(), hipMemcpyDeviceToHost, S.sA));
	HIPCHK(hipEventRecord(S.evx, S.sA));
	return GF2BV_OK;
}

// Export, first half: (mode 1: rank and pivot columns to the host, kernel-basis back-substitution,) the copies.
int finish_begin(Solver &S)
{
	if (S.mode == GF2BV_MODE_AFFINE_SPACE) {
		int rc = load_free_order(S);
		if (rc) return rc;
		std::vector<int> yc;
		if (!S.hst.inconsistent) yc = S.free_order;
		yc.push_back((int)S.cols);
		if ((rc = enqueue_backsub(S, yc))) return rc;
	}
	return enqueue_export(S);
}

// After the streams of a solve are synchronised: an expired stream hand-over gate voids the solve -- an error under flag
// synchronisation; else the device is marked and the caller runs the solve once more with events.
int handover_verdict(Solver &S)
{
	if (!S.hst.gate_timeout) return GF2BV_OK;
	if (!S.flag_sync) return fail(GF2BV_ERR_HIP, "a stream hand-over gate timed out on the device");
	forget_concurrency(S.device);
	return GF2BV_RETRY_EVENTS;
}

// The fields every result shares: status, rank (= the pivots' count), cw, dim, pivots, origin (the cw words at `origin`
// when solved, zero otherwise).  The caller adds the basis and the stats.
std::unique_ptr<gf2bv_result> new_result(bool solved, i64 cols, const int32_t *piv, i64 rank, const u64 *origin)
{
	const i64 cw = (cols + 63) / 64;
	std::unique_ptr<gf2bv_result> R(new gf2bv_result());
	R->status = solved ? GF2BV_STATUS_SOLVED : GF2BV_STATUS_INCONSISTENT;
	R->rank = rank;
	R->cw = cw;
	R->dim = cols - rank;
	R->pivots.assign(piv, piv + rank);
	R->origin.assign((size_t)std::max<i64>(1, cw), 0);
	if (solved) std::copy(origin, origin + cw, R->origin.begin());
	return R;
}

// The kernel basis out of back-substitution outputs 0 .. dim (max(1, cw) words apart): vector t is output t with the bit of
// its free column free_order[t] set.
std::vector<u64> basis_rows(const u64 *hout, i64 cw, const std::vector<int> &free_order, i64 dim)
{
	const i64 cwx = std::max<i64>(1, cw);
	std::vector<u64> basis((size_t)(dim * cwx), 0);
	for (i64 t = 0; t < dim; t++) {
		u64 *v = basis.data() + (size_t)(t * cwx);
		std::copy(hout + (size_t)(t * cwx), hout + (size_t)(t * cwx + cw), v);
		const int f = free_order[(size_t)t];
		v[f >> 6] |= 1ull << (f & 63);
	}
	return basis;
}

void fill_stats(const Solver &S, gf2bv_result *R);

// When every bulk-update launch of a finished timed solve ran, in ms from ev0: one copy of the stamps the launches left (the
// clock runs at 100 MHz), and the event pairs of the launches that have no slot.  *ok = false: the stamps could not be read, or a
// slot that was handed out is not a launch's (every launch leaves both stamps, behind the clock at ev0) -- the caller then reports a
// NEGATIVE ms_sweep and not a sum that misses launches.
std::vector<std::pair<float, float>> sweep_intervals(const Solver &S, bool *ok)
{
	if (S.sweep_read) { *ok = S.sweep_read > 0; return S.sweep_iv; }
	std::vector<std::pair<float, float>> iv;
	*ok = true;
	if (S.stamps && S.n_stamps > 1) {
		std::vector<unsigned long long> h(2 * (size_t)S.stamp_cap);
		if (hipMemcpyAsync(h.data(), S.stamps, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, S.sA) == hipSuccess
		    && hipStreamSynchronize(S.sA) == hipSuccess) {
			for (int i = 1; i < S.n_stamps; i++) {
				const unsigned long long first = h[i], last = h[S.stamp_cap + i];
				if (first == ~0ull || last < first || first < h[0]) { *ok = false; continue; }
				iv.push_back({ (float)((double)(first - h[0]) * 1e-5), (float)((double)(last - h[0]) * 1e-5) });
			}
		} else { (void)hipGetLastError(); *ok = false; }
	}
	for (size_t i = 0; i + 1 < S.kev.size(); i += 2) {
		float ms = 0, at = 0;
		(void)hipEventElapsedTime(&ms, S.kev[i], S.kev[i + 1]);
		if (hipEventElapsedTime(&at, S.ev0, S.kev[i]) != hipSuccess) { (void)hipGetLastError(); at = iv.empty() ? 0.f : iv.back().second; }
		iv.push_back({ at, at + ms });
	}
	S.sweep_iv = iv; S.sweep_read = *ok ? 1 : -1;
	return iv;
}

// Export, second half: wait for the copies and build the result object.
int finish_end(Solver &S, gf2bv_result **out)
{
	Trace tr;
	HIPCHK(hipStreamSynchronize(S.sA));
	HIPCHK(hipStreamSynchronize(S.sB));
	tr.mark(S.kn, "finish: sync");
	int rc = handover_verdict(S);
	if (rc) return rc;
	const SolveState &hst = S.hst;
	const i64 cwx = std::max<i64>(1, S.cw);
	S.hpiv.resize(hst.rank);
	std::unique_ptr<gf2bv_result> R = new_result(!hst.inconsistent, S.cols, S.hpiv.data(), hst.rank, S.hout.data() + (size_t)((S.bs.ny - 1) * cwx));
	if (!hst.inconsistent && S.mode == GF2BV_MODE_AFFINE_SPACE) R->basis = basis_rows(S.hout.data(), S.cw, S.free_order, R->dim);
	fill_stats(S, R.get());
	tr.mark(S.kn, "finish: result");
	*out = R.release();
	return GF2BV_OK;
}

// The stats of a finished solve (its streams synchronised, S.hst / S.hp on the host) into R, whose status, rank and dimension are set.
void fill_stats(const Solver &S, gf2bv_result *R)
{
	const SolveState &hst = S.hst;
	const std::vector<PanelRec> &hp = S.hp;
	const hipEvent_t evx = S.evx;
	gf2bv_stats &st = R->stats;
	st.rows = S.rows; st.cols = S.cols; st.stride_words = S.stride;
	st.rank = R->rank; st.dimension = R->dim; st.status = R->status;
	st.n_panels = S.npanels;
	st.panels_per_sweep = S.impl->G;
	st.tables_per_sweep = S.impl->G * S.impl->T;
	st.table_bits = (64 + S.impl->T - 1) / S.impl->T;          // (16-byte tiles: 8 byte fields per panel)
	st.tile_words = TW;
	st.gang_systems = S.view ? S.gang_nsys : S.nsys;
	st.search_handovers = hst.self_giveups;
	st.fast_blocks = hst.fast_blocks;
	for (int i = 0; i < 3; i++) st.sparse_blocks[i] = hst.sp_blocks[i];
	st.sparse_panels_first64 = hst.sp_first64; st.sparse_panels_absorb = hst.sp_absorb; st.sparse_panels_rounds = hst.sp_rounds;
	st.sparse_giveups = S.run.giveups;
	for (int i = 0; i < 5; i++) st.sparse_giveup_why[i] = S.run.why[i];
	st.sparse_nz_max = hst.sp_nz_max;
	st.general_unit0 = hst.gs_unit0; st.general_adopted = hst.gs_adopt; st.general_merged = hst.gs_merge;
	st.general_wide = hst.gs_wide; st.general_two_level = hst.gs_two_level;
	st.general_group_adopted = hst.gs_group_adopt; st.general_group_merged = hst.gs_group_merge;
	st.general_gj_kept = hst.gs_gj_kept; st.general_gj_redone = hst.gs_gj_redone; st.general_chunks = hst.gs_chunks;
	{
		const int G = S.impl->G;
		for (int b = 0; b < S.nblocks; b++) {
			const int j0 = b * G, gb = std::min(G, S.npanels - j0), wlo = j0 + gb;
			int pend = 0, any = 0;
			for (int g = 0; g < gb; g++) { any |= hp[j0 + g].p; pend = hp[j0 + g].start + hp[j0 + g].p; }
			if (!any || wlo >= S.wt) continue;
			const double rows_swept = (double)(S.rows - pend);
			st.n_sweeps++;
			st.sweep_words += rows_swept * (double)(S.wt - wlo);
			st.row_xors += rows_swept * (double)(S.impl->T * gb);
			// what the launches moved: a block inside an outer panel is applied by k_update16 up to the panel's end only, the
			// rest of the row takes the whole panel in one outer pass (counted at the panel's last block, two launches)
			if (S.tl_K && b < S.tl_bend) {
				const int pend_w = (b / S.tl_K + 1) * S.tl_K * G;
				const i64 out_w = S.wt;
				st.outer_blocks++;
				if (pend_w > wlo) { st.hbm_words += rows_swept * (double)(std::min<i64>(pend_w, S.wt) - wlo); st.bulk_launches++; }
				if ((b + 1) % S.tl_K == 0 && out_w > pend_w) { st.hbm_words += rows_swept * (double)(out_w - pend_w); st.bulk_launches += 2; }      // (the next panel's tiles, then the rest -- in two halves on two streams since late round 5)
			} else { st.hbm_words += rows_swept * (double)(S.wt - wlo); st.bulk_launches++; }
		}
	}
	st.ms_pack = S.ms_pack;
	st.handover_retries = g_attempt;
	(void)hipEventElapsedTime(&st.ms_eliminate, S.ev0, S.ev1);
	(void)hipEventElapsedTime(&st.ms_backsub, S.ev1, S.ev2);
	(void)hipEventElapsedTime(&st.ms_export, S.ev2, evx);
	{
		// ms_sweep = the time during which AT LEAST ONE bulk-update launch was running: launches of one stream add up as before
		// (every one-level plan), launches that run side by side -- the two halves of an outer pass on their two streams, the next
		// panel's inner updates beside them -- count once (summed, the split pass of late round 5 would be counted twice)
		bool stamps_ok = true;
		std::vector<std::pair<float, float>> iv = sweep_intervals(S, &stamps_ok);
		std::sort(iv.begin(), iv.end());
		float lo = 0, hi = -1;
		for (const auto &v : iv) {
			if (hi < 0) { lo = v.first; hi = v.second; }
			else if (v.first <= hi) hi = std::max(hi, v.second);
			else { st.ms_sweep += hi - lo; lo = v.first; hi = v.second; }
		}
		if (hi >= 0) st.ms_sweep += hi - lo;
		if (!stamps_ok) st.ms_sweep = -1.f;
	}
	st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - S.t_begin).count();
}

int solver_finish(Solver &S, gf2bv_result **out)
{
	int rc = finish_begin(S);
	if (rc) return rc;
	return finish_end(S, out);
}

// A non-owning window on system s of a gang: the gang's plan for one system, that system's matrix and side arrays.
// Back-substitution and export then run per system, unchanged.  Borrowed: the streams sA and sB and the timing events ev0, ev1,
// ev3.  Its own: ev2, evx and whatever its back-substitution allocates (unless it borrows the gang's: BackSub::borrow).
int make_view(const Solver &S, int s, Solver &V)
{
	V.plan() = S.plan();
	V.view = true;
	V.gang_nsys = S.nsys;
	V.nsys = 1; V.m_stride = 0; V.src_sys_words = 0;
	V.M = S.M + S.m_stride * s;
	V.arena = (char *)S.arena + S.lay.stride * s;
	V.bind(S.lay, V.arena, S.kn.pc);
	V.lay.stride = 0;
	V.sA = S.sA; V.sB = S.sB;
	V.ev0 = S.ev0; V.ev1 = S.ev1; V.ev3 = S.ev3;
	HIPCHK(pool().event(&V.ev2, true));
	return GF2BV_OK;
}

// One gang: S.nsys same-shape systems, forward elimination in lock-step (one set of launches),
// then back-substitution and export system by system.
int solve_gang(Solver &S, gf2bv_result **out)
{
	int rc = solver_alloc(S);
	if (rc) return rc;
	rc = enqueue_forward(S);
	if (rc) return rc;
	std::vector<Solver> V(S.nsys);
	for (int s = 0; s < S.nsys; s++) {
		V[s].device = S.device;
		rc = make_view(S, s, V[s]);
		if (rc) return rc;
	}
	if (S.mode == GF2BV_MODE_SINGLE) {
		if (!S.kn.gang_bs)      // (A/B: one chain per system, as rounds 1-3)
			for (int s = 0; s < S.nsys; s++) {
				rc = enqueue_backward_parity(V[s], { (int)S.cols });
				if (rc) return rc;
			}
		else {
			rc = enqueue_backward_parity(S, { (int)S.cols });
			if (rc) return rc;
			for (int s = 0; s < S.nsys; s++) {
				V[s].bs.borrow(S.bs, s, std::max<i64>(1, S.cw));
				HIPCHK(hipEventRecord(V[s].ev2, S.sA));
			}
		}
	}
	for (int s = 0; s < S.nsys; s++) {
		rc = finish_begin(V[s]);
		if (rc) return rc;
	}
	for (int s = 0; s < S.nsys; s++) {
		rc = finish_end(V[s], &out[s]);
		if (rc) return rc;
	}
	if (S.time_kernels) {        // one set of bulk-update launches served the whole gang: every member reports the gang's time
		float total = 0;
		bool stamps_ok = true;
		for (const auto &v : sweep_intervals(S, &stamps_ok)) total += v.second - v.first;
		if (!stamps_ok) total = -1.f;
		for (int s = 0; s < S.nsys; s++) out[s]->stats.ms_sweep = total;
	}
	return GF2BV_OK;
}

// Gang size for nsys same-shape systems (free_b: free device memory, < 0 = ask the current device).
i64 pick_gang(const Knobs &kn, i64 nsys, i64 rows, i64 cols, i64 free_bytes = -1)
{
	// gang size: ~4.5 GiB of working matrices per gang (32768^2: 32 systems -- round 4: 192 x 32768^2 run 3.22 ms per system in gangs
	// of 32 against 3.22-3.32 in gangs of 24, and 512 systems are 16 equal gangs instead of 21 + a part gang; 4096^2: 64), at
	// least four gangs (round 3, 144 x
	// 32768^2 on one box: gangs of 4 / 8 / 12 / 18 / 24 / 36 -> 231 / 248 / 250 / 239-254 / 255-256 / 255 systems per second)
	// when there are enough systems (measured on MI355X, 48 x 32768^2: gang 4/8/16 -> 7.6/6.3/6.0 ms per
	// system, one system at a time 15-28; 64 x 4096^2: 0.22 ms per system against 1.8)
	const double per_sys = 1.05 * 8.0 * (double)(rows + 64) * (double)((cols + 64) / 64 + TW + 4 * GF2_GMAX);
	i64 gang = std::max<i64>(2, std::min<i64>(64, (i64)(4.5 * 1073741824.0 / per_sys)));
	// (at least TWO gangs -- one per host thread -- where round 3 asked for four: with a system per XCD larger gangs win; a rank's share of
	// the configs[3] job at 8 GPUs, 64 x 32768^2: 2 x 32 run 3.25 ms per system against 3.41 for 4 x 16, profiles/r05_batch_scans.txt)
	gang = std::min(gang, std::max<i64>(1, (nsys + 1) / 2));
	// equal gangs, an even number of them (two host threads take alternate gangs): 64 systems of 32768^2 go as 4 x 16
	// (3.90 ms per system) rather than 4 x 14 + 8 (4.10)
	if (gang < nsys) {
		i64 ngangs = (nsys + gang - 1) / gang;
		if (ngangs > 1 && (ngangs & 1)) ngangs++;
		gang = (nsys + ngangs - 1) / ngangs;
	}
	// whole multiples of 8 systems: the bulk update of such a gang keeps every system on ONE XCD (k_update16: xcd_nsys)
	if (gang >= 8) gang = gang / 8 * 8;
	if (kn.gang >= 1) gang = kn.gang;
	gang = std::max<i64>(1, std::min<i64>(gang, nsys));
	{
		size_t free_b = 0, total_b = 0;
		if (free_bytes >= 0) gang = std::max<i64>(1, std::min<i64>(gang, (i64)(0.4 * (double)free_bytes / per_sys)));
		else if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
			gang = std::max<i64>(1, std::min<i64>(gang, (i64)(0.4 * (double)free_b / per_sys)));
	}
	return gang;
}

// fn(0) on the calling thread, fn(1) .. fn(n - 1) on threads of their own, each under the exception policy of guarded(); returns
// the first failure with its message.
template <class F>
int run_on_threads(int n, F &&fn)
{
	std::mutex mu;
	int rc = GF2BV_OK;
	std::string why;
	auto one = [&](int t) {
		const int r = catching([&] { return fn(t); });
		std::lock_guard<std::mutex> lk(mu);
		if (r != GF2BV_OK && rc == GF2BV_OK) { rc = r; why = g_err; }
	};
	bool started = true;
	{
		std::vector<std::thread> th;
		struct Join { std::vector<std::thread> &w; ~Join() { for (auto &t : w) t.join(); } } joiner{ th };
		try { for (int t = 1; t < n; t++) th.emplace_back(one, t); }
		catch (const std::exception &) { started = false; }
		if (started && n > 0) one(0);
	}
	if (!started) return fail(GF2BV_ERR_NOMEM, "could not start a host thread");
	return rc == GF2BV_OK ? GF2BV_OK : fail(rc, why.c_str());
}

// The gangs of a batch call: nsys same-shape systems in gangs of `gang` (the last one may be shorter), results into out[0..nsys),
// which are null on entry.  Host threads (2 by default, GF2BV_BATCH_THREADS: 1 .. 16) each take a class-2 pool stream that
// waits for `ready` and, when worker_bytes > 0, that many bytes of device memory; then they claim gangs in order from one
// counter -- one gang's back-substitution, export and staging overlap another's elimination.  stage(S, s0, ns, buf) puts
// systems s0 .. s0 + ns into the fresh Solver S on the worker's stream S.sA (shape, mode, and S.src or a filled S.M); solve_gang
// does the rest, and the stream is synchronised after every gang (stage may reuse buf).  After the first failure no more
// gangs are claimed and that failure is returned, every out[s] null.
// Two threads that start together stay in phase for the whole job -- both gangs bulk-bound at once, both in their tails at
// once.  Starting them apart (the list beginning with part gangs, thread t's first gang (t + 1) / NS of a full one) was built
// and measured in round 4: 3.56 ms per system against 3.42 in phase on 192 x 32768^2 (profiles/r04_batch_scans.txt) -- the
// bulk update runs throughout a gang's elimination (its launches are in flight 89 % of the wall time), there is no idle tail
// to fill, and part gangs only make smaller launches.
template <class Stage>
int run_gangs(const Knobs &kn, int device, i64 nsys, i64 gang, hipEvent_t ready, size_t worker_bytes, gf2bv_result **out, Stage &&stage)
{
	const i64 ngangs = (nsys + gang - 1) / gang;
	std::atomic<i64> next_gang{0};
	auto work = [&]() -> int {
		Held W(device);
		void *buf = nullptr;
		HIPCHK(hipSetDevice(device));
		HIPCHK(W.stream(2));
		HIPCHK(hipStreamWaitEvent(W.st, ready, 0));
		if (worker_bytes) HIPCHK(W.get(&buf, worker_bytes));
		for (i64 q; (q = next_gang.fetch_add(1)) < ngangs;) {
			const i64 s0 = q * gang;
			const int ns = (int)std::min<i64>(gang, nsys - s0);
			// an expired hand-over gate voids THIS gang only: guarded() runs it once more with events (the device is marked by
			// then; g_attempt is its members' handover_retries), after dropping what the voided attempt built
			const int rc = guarded([&]() -> int {
				for (int k = 0; k < ns; k++) { delete out[s0 + k]; out[s0 + k] = nullptr; }
				Solver S;
				S.t_begin = std::chrono::steady_clock::now();
				S.device = device;
				S.sA = W.st;
				S.nsys = ns;
				const int r = stage(S, s0, ns, buf);
				return r ? r : solve_gang(S, &out[s0]);
			});
			if (rc) return rc;
			HIPCHK(hipStreamSynchronize(W.st));
		}
		return GF2BV_OK;
	};
	const int rc = run_on_threads((int)std::min<i64>(ngangs, kn.batch_threads), [&](int) {
		const int r = work();
		if (r) next_gang.store(ngangs);
		return r;
	});
	if (rc) for (i64 s = 0; s < nsys; s++) { delete out[s]; out[s] = nullptr; }
	return rc;
}

int check_shape(i64 rows, i64 cols, int mode)
{
	// mirrors gf2bv/_internal.c:372-395
	if (cols <= 0) return fail(GF2BV_ERR_ARG, "Number of columns must be positive");
	if (mode != GF2BV_MODE_SINGLE && mode != GF2BV_MODE_AFFINE_SPACE) return fail(GF2BV_ERR_ARG, "Invalid mode");
	if (rows < cols)
		return fail(GF2BV_ERR_ARG, "Number of rows must be greater than or equal to number of columns, try pad with zeros.");
	if (rows >= (1ll << 31) - 64 || cols >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, "system too large");
	return GF2BV_OK;
}

// One matrix as the single-system entries take it, in one of three forms: d_words (device, row-major, `stride` words apart)
// | h_words (host, row-major, `stride` words apart) | h_digits + h_off (host, bpd bits per digit, row r = digits
// h_off[r] .. h_off[r + 1]).  The form is the one whose pointer is set (the digits form: h_off; h_digits may be null when
// there are no digits).
struct MatrixInput {
	const u64 *d_words = nullptr, *h_words = nullptr;
	i64 stride = 0;
	const uint32_t *h_digits = nullptr;
	const i64 *h_off = nullptr;
	int bpd = 0;
};

// The argument checks of a matrix, made before any device is touched: the shape, then those of the form in use (no form
// pointer set: the caller passed a null matrix)
int check_matrix_form(const MatrixInput &in, i64 rows, i64 cols);
int check_matrix_input(const MatrixInput &in, i64 rows, i64 cols, int mode)
{
	int rc = check_shape(rows, cols, mode);
	if (rc) return rc;
	return check_matrix_form(in, rows, cols);
}

// The digits form of nrows rows: bits per digit, offsets that start at 0 (`from_zero`: a batch's offsets are absolute, a share
// of a larger batch starts where the one before it ends) and never decrease, and digits wherever the offsets say there are some
int check_digit_rows(const uint32_t *digits, const i64 *off, i64 nrows, int bpd, bool from_zero)
{
	if (bpd < 1 || bpd > 32) return fail(GF2BV_ERR_ARG, "bits_per_digit must be 1..32");
	if (from_zero && off[0] != 0) return fail(GF2BV_ERR_ARG, "digit offsets must start at 0");
	for (i64 r = 0; r < nrows; r++)
		if (off[r + 1] < off[r]) return fail(GF2BV_ERR_ARG, "digit offsets must not decrease");
	if (!digits && off[nrows] > off[0]) return fail(GF2BV_ERR_ARG, "null pointer");
	return GF2BV_OK;
}

// The checks of the form in use alone (an append has shape rules of its own: check_append_args)
int check_matrix_form(const MatrixInput &in, i64 rows, i64 cols)
{
	const i64 wt = (cols + 1 + 63) / 64;
	if (in.h_off)
		return check_digit_rows(in.h_digits, in.h_off, rows, in.bpd, true);
	else if (in.h_words) {
		if (in.stride < wt) return fail(GF2BV_ERR_ARG, "stride_words does not cover cols+1 bits");
	} else if (in.d_words) {
		if (in.stride % 2 != 0 || in.stride < wt || ((uintptr_t)in.d_words & 15))
			return fail(GF2BV_ERR_ARG, "device matrix needs 16-byte alignment and an even stride_words covering cols+1 bits");
	} else
		return fail(GF2BV_ERR_ARG, "null pointer");
	return GF2BV_OK;
}

// The argument checks of the digits batch entries, in the single entries' order: out (then out[0..nsys) cleared), the shape,
// the form of all nsys * rows rows
int check_digits_batch(const uint32_t *digits, const int64_t *off, int bpd, i64 nsys, i64 rows, i64 cols, int mode, gf2bv_result **out)
{
	if (!out || nsys < 0) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 s = 0; s < nsys; s++) out[s] = nullptr;
	const int rc = check_shape(rows, cols, mode);
	if (rc) return rc;
	if (!off) return fail(GF2BV_ERR_ARG, "null pointer");
	return check_digit_rows(digits, reinterpret_cast<const i64 *>(off), nsys * rows, bpd, false);
}

// ---- small systems: the whole solve in one launch (k_small_solve) ---------------------------------------------------
// Eligible: the augmented matrix + two sets of nibble tables fit the LDS of one workgroup ((rows + 512) x odd row pitch <= 18432 words = 144 KiB, cols <= 1023,
// rows <= 4096).  Per call: ONE host-to-device copy out of a pinned staging buffer (offsets + digits, or the packed words;
// none when the matrix already lives on the device), one launch, and the result written by the kernel straight into pinned
// host memory -- no device-to-host copy.  GF2BV_SMALL=0 sends these systems down the blocked path instead (tests compare both).
struct SmallStage {            // pinned staging of one call in flight (input copy / zero-copy source, and the result)
	int device = -1;
	char *h_in = nullptr, *h_out = nullptr;
	size_t in_cap = 0, out_cap = 0;
};
// Stages are handed out per call and go back afterwards: as many exist as calls were ever in flight at once on a device (a
// thread_local pair per host thread would pin 320 KiB for every thread a pool ever creates).  Never freed at exit: the HIP runtime
// may be gone by then.
struct StagePool {
	std::mutex mu;
	std::map<int, std::vector<SmallStage *>> idle;
	SmallStage *take(int device)
	{
		std::lock_guard<std::mutex> lk(mu);
		auto &v = idle[device];
		if (!v.empty()) { SmallStage *s = v.back(); v.pop_back(); return s; }
		SmallStage *s = new SmallStage();
		s->device = device;
		return s;
	}
	void give(SmallStage *s) { std::lock_guard<std::mutex> lk(mu); idle[s->device].push_back(s); }
};
StagePool &stage_pool() { static StagePool *p = new StagePool(); return *p; }

bool small_eligible(const Knobs &kn, i64 rows, i64 cols)
{
	const i64 wt = (cols + 1 + 63) / 64;
	return kn.small && cols <= GF2_SMALL_MAXCOLS && rows <= GF2_SMALL_MAXROWS && (rows + 512) * small_pitch(wt) <= GF2_SMALL_LDS_WORDS;
}

int small_stage(SmallStage &G, size_t in_bytes, size_t out_bytes)
{
	if (in_bytes > G.in_cap) {
		if (G.h_in) (void)hipHostFree(G.h_in);
		G.h_in = nullptr; G.in_cap = 0;
		const size_t cap = std::max<size_t>(in_bytes * 2, (size_t)256 << 10);
		HIPCHK(hipHostMalloc((void **)&G.h_in, cap, hipHostMallocDefault));
		G.in_cap = cap;
	}
	if (out_bytes > G.out_cap) {
		if (G.h_out) (void)hipHostFree(G.h_out);
		G.h_out = nullptr; G.out_cap = 0;
		const size_t cap = std::max<size_t>(out_bytes * 2, (size_t)64 << 10);
		HIPCHK(hipHostMalloc((void **)&G.h_out, cap, hipHostMallocDefault));
		G.out_cap = cap;
	}
	return GF2BV_OK;
}

int small_solve(const Knobs &kn, const MatrixInput &in, i64 rows, i64 cols, int mode, int device, hipStream_t stream, gf2bv_result **out)
{
	const auto t_begin = std::chrono::steady_clock::now();
	const i64 wt = (cols + 1 + 63) / 64, cw = (cols + 63) / 64;
	const bool want_basis = mode == GF2BV_MODE_AFFINE_SPACE;
	const size_t head = 16 + 4 * (size_t)((cols + 1) & ~(i64)1);
	const size_t res_bytes = head + 8 * (size_t)cw * (1 + (want_basis ? (size_t)cols : 0));
	const size_t out_bytes = res_bytes + 64;                 // (+ 8 phase counters of the probe, GF2BV_SMALL_PROBE=1)
	size_t in_bytes = 0;
	i64 ndig = 0;
	if (in.h_off) { ndig = in.h_off[rows]; in_bytes = sizeof(i64) * (size_t)(rows + 1) + sizeof(uint32_t) * (size_t)std::max<i64>(ndig, 1); }
	else if (in.h_words) in_bytes = sizeof(u64) * (size_t)(rows * wt);
	struct Stage { SmallStage *s; ~Stage() { stage_pool().give(s); } } stage{ stage_pool().take(device) };
	SmallStage &G = *stage.s;
	int rc = small_stage(G, in_bytes, out_bytes);
	if (rc) return rc;
	// Stream: a matrix that already lives on the device is whatever `stream` (NULL = the null stream) has produced -- the launch goes
	// onto that very stream, as on the blocked path.  Host inputs depend on nothing: a pool stream of their own (non-blocking).
	Held H(device);
	if (!stream && !in.d_words) HIPCHK(H.stream(0)); else H.on(stream);
	const hipStream_t st = H.st;
	void *d_in = nullptr;
	const u64 *d_src = in.d_words;
	i64 d_stride = in.stride;
	const uint32_t *d_dig = nullptr;
	const i64 *d_off = nullptr;
	// inputs up to 32 KiB: no copy at all -- the kernel reads the pinned staging buffer over the link (two batched round trips;
	// 2-6 us less than a host-to-device copy in front of the launch: profiles/r04_small.txt).  GF2BV_SMALL_ZC=0 / 1 forces either.
	const bool zero_copy = kn.small_zc >= 0 ? kn.small_zc != 0 : in_bytes <= ((size_t)32 << 10);
	if (in_bytes) {
		if (!zero_copy) HIPCHK(H.get(&d_in, in_bytes));
		char *d_base = zero_copy ? G.h_in : (char *)d_in;
		if (in.h_off) {
			memcpy(G.h_in, in.h_off, sizeof(i64) * (size_t)(rows + 1));
			if (ndig) memcpy(G.h_in + sizeof(i64) * (size_t)(rows + 1), in.h_digits, sizeof(uint32_t) * (size_t)ndig);
			d_off = (const i64 *)d_base;
			d_dig = (const uint32_t *)(d_base + sizeof(i64) * (size_t)(rows + 1));
		} else {
			for (i64 r = 0; r < rows; r++) memcpy(G.h_in + sizeof(u64) * (size_t)(r * wt), in.h_words + r * in.stride, sizeof(u64) * (size_t)wt);
			d_src = (const u64 *)d_base; d_stride = wt;
		}
		if (!zero_copy) HIPCHK(hipMemcpyAsync(d_in, G.h_in, in_bytes, hipMemcpyHostToDevice, st));
	}
	// 16 wavefronts: every phase but wavefront 0's column loop is a few dependent LDS round trips per item, i.e. latency --
	// 640 x 256: 143 us with 256 threads (profiles/r04_small.txt)
	constexpr int NT = 1024;
	const size_t lds = sizeof(u64) * (size_t)((rows + 512) * small_pitch(wt)) + sizeof(SmallLds);
	{
		static std::mutex mu;
		static std::map<int, bool> raised;          // device -> the > 64 KiB dynamic-LDS attribute has been raised there
		std::lock_guard<std::mutex> lk(mu);
		if (!raised[device]) {
			HIPCHK(hipFuncSetAttribute((const void *)k_small_solve<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
			raised[device] = true;
		}
	}
	memset(G.h_out, 0, 16);
	k_small_solve<NT><<<dim3(1), dim3(NT), lds, st>>>(d_src, d_stride, d_dig, d_off, in.bpd, (int)rows, (int)cols, want_basis ? 1 : 0, (unsigned *)G.h_out,
	                                                   kn.small_probe ? (unsigned long long *)(G.h_out + res_bytes) : nullptr);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(st));
	const unsigned *ho = (const unsigned *)G.h_out;
	if (kn.small_probe) {
		const unsigned long long *p = (const unsigned long long *)(G.h_out + res_bytes);
		fprintf(stderr, "[gf2bv small %lld x %lld] us: load %.1f candidates %.1f wavefront0 %.1f candidate rows %.1f tables %.1f all rows %.1f read-out %.1f; passes %llu\n",
		        (long long)rows, (long long)cols, p[0] / 100.0, p[1] / 100.0, p[2] / 100.0, p[3] / 100.0, p[4] / 100.0, p[5] / 100.0, p[6] / 100.0, p[7]);
	}
	const i64 rank = ho[0];
	const bool bad = ho[1] != 0;
	if (rank < 0 || rank > cols) return fail(GF2BV_ERR_HIP, "small solve returned an impossible rank");
	const int32_t *pv = (const int32_t *)(G.h_out + 16);
	const u64 *org = (const u64 *)(G.h_out + head);
	std::unique_ptr<gf2bv_result> R = new_result(!bad, cols, pv, rank, org);
	if (!bad && want_basis) {
		// the kernel wrote the vectors in ascending column order: vector t is the one of free column free_order[t]
		const std::vector<int> free_order = m4ri_free_order(pv, rank, cols);
		std::vector<int> slot(cols, -1);
		std::vector<char> isp(cols, 0);
		for (i64 i = 0; i < rank; i++) isp[pv[i]] = 1;
		int j = 0;
		for (i64 c = 0; c < cols; c++) if (!isp[c]) slot[c] = j++;
		const u64 *Y = org + cw;
		R->basis.assign((size_t)R->dim * std::max<i64>(1, cw), 0);
		for (i64 t = 0; t < R->dim; t++) {
			const int f = free_order[(size_t)t];
			u64 *v = R->basis.data() + (size_t)t * cw;
			std::copy(Y + (size_t)slot[f] * cw, Y + (size_t)(slot[f] + 1) * cw, v);
			v[f >> 6] |= 1ull << (f & 63);
		}
	}
	gf2bv_stats &s = R->stats;
	s.rows = rows; s.cols = cols; s.stride_words = wt;
	s.rank = rank; s.dimension = R->dim; s.status = R->status;
	s.n_panels = (int)cw; s.gang_systems = 1; s.tile_words = 0;
	s.small_path = 1;
	s.small_passes = (int32_t)(ho[3] & 0xFFFFu); s.small_pass_kinds = (int32_t)(ho[3] >> 16);
	s.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
	*out = R.release();
	return GF2BV_OK;
}

// ---- many right-hand sides of one matrix: ONE elimination for all of them ---------------------------------------------------
// The reference factors A alone -- A (rows x cols) and B (rows x 1) are separate mzd_t, _mzd_pluq(A, P, Q) runs on A
// (_internal.c:398-433), and only then is B solved against (:438-455) -- so pivots, the origin rule (free variables 0) and the
// kernel basis depend on A only; a right-hand side decides consistency and the origin.  Here right-hand side j is column cols + j
// of the working matrix (ceil((cols + nrhs) / 64) words per row): the elimination carries every one of them along, k_check_rhs_many
// decides every system's consistency, and one back-substitution over U yields every origin (mode 1: and the kernel basis, once).
// Scope: one system on one device (no gangs, no column slabs); every size takes the blocked path -- k_small_solve's LDS budget
// assumes one RHS bit.
// The argument checks of the right-hand sides of a gf2bv_solve_rhs_* entry, made before any device is touched (the matrix's
// come first: check_matrix_input)
int check_rhs_args(i64 rows, i64 cols, const void *rhs, bool on_device, i64 nrhs, i64 rhs_words)
{
	if (!rhs) return fail(GF2BV_ERR_ARG, "null pointer");
	if (nrhs < 1) return fail(GF2BV_ERR_ARG, "nrhs must be at least 1");
	if (nrhs >= (1ll << 31) - 64 - cols) return fail(GF2BV_ERR_ARG, "too many right-hand sides");
	if (rhs_words < (rows + 63) / 64) return fail(GF2BV_ERR_ARG, "rhs_words does not cover one bit per row");
	if (on_device && ((uintptr_t)rhs & 7)) return fail(GF2BV_ERR_ARG, "the right-hand sides need 8-byte alignment");
	return GF2BV_OK;
}

// The coefficients into the tile-major working matrix (ntiles tiles, srows rows per slab) on stream `st`: the digits packed straight into
// tiles (k_pack_digits puts the affine term at column `cols`; the callers overwrite it), or the words that hold coefficients -- and
// only those -- copied into tiles (the words right of them are zero-filled)
// (M: where row 0 goes -- an append packs its rows below the kept ones by passing S.M + row0 x TW)
int pack_coefficients(const MatrixInput &in, i64 rows, i64 cols, i64 ntiles, i64 srows, hipStream_t st, Held &held, u64 *M)
{
	const i64 cw = (cols + 63) / 64, rw = (rows + 63) / 64;
	if (in.h_off) {
		const i64 ndig = in.h_off[rows];
		uint32_t *d_dig = nullptr;
		i64 *d_off = nullptr;
		HIPCHK(held.get((void **)&d_dig, sizeof(uint32_t) * std::max<i64>(1, ndig)));
		HIPCHK(held.get((void **)&d_off, sizeof(i64) * (rows + 1)));
		if (ndig) HIPCHK(hipMemcpyAsync(d_dig, in.h_digits, sizeof(uint32_t) * ndig, hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d_off, in.h_off, sizeof(i64) * (rows + 1), hipMemcpyHostToDevice, st));
		k_pack_digits<<<dim3((unsigned)((ntiles * TW + 255) / 256), (unsigned)std::min<i64>(rows, 65535)), dim3(256), 0, st>>>(
			d_dig, d_off, in.bpd, rows, cols, ntiles * TW, srows, M, SysStride{0, 0}, (i64)0);
	} else {
		const u64 *src = in.d_words;
		i64 sstride = in.stride;
		if (in.h_words) {
			sstride = round_up(cw, 2);
			u64 *tmp = nullptr;
			HIPCHK(held.get((void **)&tmp, sizeof(u64) * rows * sstride));
			HIPCHK(hipMemcpy2DAsync(tmp, sstride * 8, in.h_words, in.stride * 8, cw * 8, rows, hipMemcpyHostToDevice, st));
			src = tmp;
		}
		k_to_tiled<<<dim3((unsigned)rw, (unsigned)((ntiles + 15) / 16)), dim3(256), 0, st>>>(src, sstride, rows, ntiles, cw, srows, M,
		                                                                                      (i64)0, SysStride{0, 0});
	}
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

int solve_rhs(const MatrixInput &in, const u64 *rhs, bool rhs_on_device, i64 nrhs, i64 rhs_words, i64 rows, i64 cols, int mode, int device,
              hipStream_t stream, bool time_kernels, gf2bv_result **out)
{
	const i64 cw = (cols + 63) / 64, cwx = std::max<i64>(1, cw), nmw = (nrhs + 63) / 64;
	const i64 wt = (cols + nrhs + 63) / 64, ntiles = tiles_for(wt), srows = slab_rows(rows);
	const i64 rw = (rows + 63) / 64, nrw = ((cols & 63) + nrhs + 63) / 64;
	Solver S;
	S.t_begin = std::chrono::steady_clock::now();
	S.device = device;
	if (in.d_words) S.sA = stream;
	else { HIPCHK(pool().stream(&S.sA, device, false)); S.own_sA = true; }
	S.rows = rows; S.cols = cols; S.mode = mode; S.nrhs = (int)nrhs;
	S.time_kernels = time_kernels;
	S.stride = in.h_off ? ntiles * TW : in.stride;
	if (int rc = alloc_or_nomem((void **)&S.M, sizeof(u64) * ntiles * TW * srows + kOuterSlackBytes, device,
	                            "the matrix widened by the right-hand sides does not fit on the device", "working matrix")) return rc;
	Held held(device, S.sA);                // (declared after S: what the entry holds goes back before what the solver owns)
	HIPCHK(held.get((void **)&S.rhs_bad, sizeof(u64) * nmw));
	hipEvent_t p0, p1;
	HIPCHK(held.event(&p0)); HIPCHK(held.event(&p1));
	HIPCHK(hipEventRecord(p0, S.sA));
	HIPCHK(hipMemsetAsync(S.rhs_bad, 0, sizeof(u64) * nmw, S.sA));
	int rc;
	if ((rc = pack_coefficients(in, rows, cols, ntiles, srows, S.sA, held, S.M))) return rc;
	const u64 *d_rhs = rhs;
	i64 rhs_stride = rhs_words;
	if (!rhs_on_device) {             // (only the words that hold rows go up)
		u64 *d = nullptr;
		HIPCHK(held.get((void **)&d, sizeof(u64) * nrhs * rw));
		HIPCHK(hipMemcpy2DAsync(d, rw * 8, rhs, rhs_words * 8, rw * 8, nrhs, hipMemcpyHostToDevice, S.sA));
		d_rhs = d; rhs_stride = rw;
	}
	k_pack_rhs<<<dim3((unsigned)((rw + 3) / 4), (unsigned)std::min<i64>(nrw, 65535)), dim3(256), 0, S.sA>>>(d_rhs, nrhs, rhs_stride, rows, cols,
	                                                                                                  srows, S.M);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(p1, S.sA));
	rc = solver_alloc(S);             // (S.src is null: the matrix is in place)
	if (rc) return rc;
	rc = enqueue_forward(S);
	if (rc) return rc;
	// back-substitution: Y columns = [free columns in M4RI order (mode 1, once, when some system is consistent)] + every RHS column
	std::vector<u64> bad((size_t)nmw, 0);
	std::vector<int> yc;
	if (mode == GF2BV_MODE_AFFINE_SPACE) {
		if ((rc = load_free_order(S))) return rc;            // (synchronises the stream: the mask is complete)
		HIPCHK(hipMemcpy(bad.data(), S.rhs_bad, sizeof(u64) * nmw, hipMemcpyDeviceToHost));
		bool any_ok = false;
		for (i64 j = 0; j < nrhs && !any_ok; j++) any_ok = !((bad[(size_t)(j >> 6)] >> (j & 63)) & 1);
		if (any_ok) yc = S.free_order;
	}
	const i64 nbasis = (i64)yc.size();
	for (i64 j = 0; j < nrhs; j++) yc.push_back((int)(cols + j));
	if ((rc = enqueue_backsub(S, yc))) return rc;
	HIPCHK(hipMemcpyAsync(bad.data(), S.rhs_bad, sizeof(u64) * nmw, hipMemcpyDeviceToHost, S.sA));
	if ((rc = enqueue_export(S))) return rc;
	HIPCHK(hipStreamSynchronize(S.sA));
	HIPCHK(hipStreamSynchronize(S.sB));
	if ((rc = handover_verdict(S))) return rc;
	(void)hipEventElapsedTime(&S.ms_pack, p0, p1);
	S.hpiv.resize(S.hst.rank);
	// (nbasis == dim when some system is consistent in mode 1)
	const std::vector<u64> basis = basis_rows(S.hout.data(), cw, S.free_order, nbasis);
	std::vector<std::unique_ptr<gf2bv_result>> res((size_t)nrhs);
	for (i64 j = 0; j < nrhs; j++) {
		const bool ok = !((bad[(size_t)(j >> 6)] >> (j & 63)) & 1);
		res[(size_t)j] = new_result(ok, cols, S.hpiv.data(), S.hst.rank, S.hout.data() + (size_t)((nbasis + j) * cwx));
		if (ok && mode == GF2BV_MODE_AFFINE_SPACE) res[(size_t)j]->basis = basis;
		fill_stats(S, res[(size_t)j].get());
	}
	for (i64 j = 0; j < nrhs; j++) out[j] = res[(size_t)j].release();
	return GF2BV_OK;
}


// ---- a kept factorization: factor once, solve new right-hand sides later (gf2bv_factor_*) ---------------------------------
// The reference's own split (_internal.c:431-447: _mzd_pluq on A, then _mzd_pluq_solve_left on B) with the factorization kept.
// What is kept is the working matrix after eliminating [A | 0 (C slots) | I]: U in the coefficient columns and, in the identity's
// columns, the transform T that the row operations made of the identity -- rows x rows bits, as much as the matrix again when
// rows == cols.  Row operations are linear and blind to every column from `cols` on (pivots are searched in columns < cols only),
// so T b is exactly what the elimination would have left of right-hand side b in every row, whichever path eliminated each block
// (dense search, sparse search, general panel steps, a poisoned block resumed, outer panels).  A solve pass (up to C right-hand
// sides) is then one launch for T b over T plus a slot write, followed by what gf2bv_solve_rhs_* does after its elimination:
// k_check_rhs_many, the back-substitution with ycols = cols + j, the export.  Mode 1: the kernel basis depends on A alone and is
// computed once, at factor time.
}  // namespace

struct gf2bv_factor {
	mutable std::mutex mu;            // one call on a handle at a time, getters included (the binding drops the GIL)
	Solver S;                         // M = [U | slots | T], arena (pivots, urow, panel records), streams
	i64 rows = 0, cols = 0, tw0 = 0, rw = 0, cw = 0;
	int mode = 0, device = 0;
	i64 rank = 0;
	std::vector<int32_t> piv;
	std::vector<u64> basis;           // mode 1: dim x max(1, cw) words, M4RI's order (empty in mode 0)
	gf2bv_stats fst{};                // the factorization's elimination counters (copied into every result)
	i64 device_bytes = 0;
	// appends (gf2bv_factor_append_*): M has room for cap_rows rows (slab_rows(cap_rows) per slab, T columns for all of them);
	// the host copies of the panel records and the pivot rows follow every merge
	i64 cap_rows = 0;
	std::vector<PanelRec> hp;
	std::vector<int32_t> urow;
	int *died_buf = nullptr;          // per row, once the rows have outgrown the arena's (owned; S.died points here then)
	bool failed = false;              // an append failed after it had started to change the kept state: every later call refuses
	~gf2bv_factor()
	{
		if (died_buf) {
			(void)hipSetDevice(device);
			if (S.sA) (void)hipStreamSynchronize(S.sA);
			pool().release(died_buf);
		}
	}
};

namespace {

constexpr i64 kFactorSlots = 64;      // right-hand sides per solve pass (the slot columns cols .. cols + 63)
const char *kFailedHandle = "the handle is unusable: an append failed after it had started to change it";

// A kept handle keeps its solver between calls: what a back-substitution on it took from the pool goes back on every return path
struct BackSubScope {
	Solver &S;
	~BackSubScope() { S.bs.release(S.sA); }
};

// The kernel basis of a kept factorization (mode 1) from its pivots: the free columns in M4RI's order, one back-substitution over
// them.
int factor_basis(gf2bv_factor *h, std::vector<u64> &basis)
{
	Solver &S = h->S;
	basis.clear();
	int rc = load_free_order(S);
	if (rc) return rc;
	const i64 dim = h->cols - h->rank;
	if (!dim) return GF2BV_OK;
	BackSubScope scope{ S };
	if ((rc = enqueue_backsub(S, S.free_order))) return rc;
	std::vector<u64> hout((size_t)(dim * std::max<i64>(1, h->cw)));
	HIPCHK(hipMemcpyAsync(hout.data(), S.bs.out, sizeof(u64) * hout.size(), hipMemcpyDeviceToHost, S.sA));
	HIPCHK(hipStreamSynchronize(S.sA));
	basis = basis_rows(hout.data(), h->cw, S.free_order, dim);
	return GF2BV_OK;
}

// device memory a kept factorization holds: the working matrix, the arena and, once the rows have outgrown the arena's, its own row records
i64 factor_device_bytes(const gf2bv_factor *h)
{
	const Solver &S = h->S;
	return (i64)(sizeof(u64) * S.ntiles * TW * S.srows + kOuterSlackBytes + S.lay.stride) + (h->died_buf ? (i64)sizeof(int) * h->cap_rows : 0);
}

int factor_matrix(const MatrixInput &in, i64 rows, i64 cols, int mode, int device, hipStream_t stream, gf2bv_factor **out)
{
	const i64 rw = (rows + 63) / 64, cw = (cols + 63) / 64;
	const i64 tw0 = round_up(cols + kFactorSlots, 128) / 64;          // (the identity starts on a whole 16-byte tile)
	const i64 wt = tw0 + rw, ntiles = tiles_for(wt), srows = slab_rows(rows);
	std::unique_ptr<gf2bv_factor> h(new gf2bv_factor());
	h->rows = rows; h->cols = cols; h->mode = mode; h->device = device; h->tw0 = tw0; h->rw = rw; h->cw = cw;
	Solver &S = h->S;
	S.t_begin = std::chrono::steady_clock::now();
	S.device = device;
	HIPCHK(pool().stream(&S.sA, device, false));
	S.own_sA = true;
	S.rows = rows; S.cols = cols; S.mode = mode;
	S.nrhs = (int)(wt * 64 - cols);   // (solver_alloc: wt words per row)
	S.stride = in.h_off ? ntiles * TW : in.stride;
	// Ordering contract: the matrix is whatever `stream` (the caller's stream, NULL = the null stream) has produced when this
	// call is made.  S.sA is one of the library's own non-blocking streams, which is not ordered against any other stream by
	// itself: it waits for an event recorded on `stream` here.
	Held held(device, S.sA);
	if (in.d_words) {
		hipEvent_t e = nullptr;
		HIPCHK(held.event(&e, false));
		HIPCHK(hipEventRecord(e, stream));
		HIPCHK(hipStreamWaitEvent(S.sA, e, 0));
	}
	if (int rc = alloc_or_nomem((void **)&S.M, sizeof(u64) * ntiles * TW * srows + kOuterSlackBytes, device,
	                            "the factorization (the matrix and its row transform, about twice the matrix) does not fit on the device", "working matrix")) return rc;
	int rc = pack_coefficients(in, rows, cols, ntiles, srows, S.sA, held, S.M);
	if (rc) return rc;
	k_factor_init<<<dim3((unsigned)((rows + 255) / 256), (unsigned)std::min<i64>(wt - (cols >> 6), 64)), dim3(256), 0, S.sA>>>(
		rows, cols, srows, tw0, rw, S.M);
	HIPCHK(hipGetLastError());
	if ((rc = solver_alloc(S))) return rc;
	if ((rc = enqueue_forward(S))) return rc;
	// (the slots are zero: k_check_rhs finds the factorization consistent -- nothing reads that)
	HIPCHK(hipMemcpyAsync(&S.hst, S.st, sizeof S.hst, hipMemcpyDeviceToHost, S.sA));
	S.hp.resize(std::max(1, S.npanels));
	HIPCHK(hipMemcpyAsync(S.hp.data(), S.panels, sizeof(PanelRec) * S.hp.size(), hipMemcpyDeviceToHost, S.sA));
	HIPCHK(hipStreamSynchronize(S.sA));
	HIPCHK(hipStreamSynchronize(S.sB));
	if (S.sC) HIPCHK(hipStreamSynchronize(S.sC));
	if ((rc = handover_verdict(S))) return rc;
	h->rank = S.hst.rank;
	h->piv.resize((size_t)h->rank);
	h->urow.resize((size_t)h->rank);
	if (h->rank) HIPCHK(hipMemcpy(h->piv.data(), S.pivcol, sizeof(int) * h->rank, hipMemcpyDeviceToHost));
	if (h->rank) HIPCHK(hipMemcpy(h->urow.data(), S.urow, sizeof(int) * h->rank, hipMemcpyDeviceToHost));
	h->hp.assign(S.hp.begin(), S.hp.begin() + S.npanels);
	h->cap_rows = rows;
	if (mode == GF2BV_MODE_AFFINE_SPACE && (rc = factor_basis(h.get(), h->basis))) return rc;
	{
		gf2bv_result R;
		R.rank = h->rank; R.dim = cols - h->rank;
		fill_stats(S, &R);
		(void)hipGetLastError();      // (fill_stats' elapsed times of events a factorization does not record)
		h->fst = R.stats;
	}
	h->device_bytes = factor_device_bytes(h.get());
	*out = h.release();
	return GF2BV_OK;
}

// one solve pass: right-hand sides j0 .. j0 + np of rhs (device, rhs_stride words apart) into results out[0 .. np)
int factor_pass(gf2bv_factor *h, const u64 *d_rhs, i64 np, i64 rhs_stride, hipEvent_t ev[5], std::chrono::steady_clock::time_point t0,
                u64 *acc, u64 *bad, gf2bv_result **out)
{
	Solver &S = h->S;
	const i64 rows = h->rows, cols = h->cols, cw = h->cw, cwx = std::max<i64>(1, cw), rw = h->rw;
	HIPCHK(hipMemsetAsync(acc, 0, sizeof(u64) * std::max<i64>(1, rows), S.sA));
	HIPCHK(hipMemsetAsync(bad, 0, sizeof(u64), S.sA));
	HIPCHK(hipEventRecord(ev[1], S.sA));
	const unsigned gx = (unsigned)((rows + 255) / 256);
	k_apply_transform<<<dim3(gx, (unsigned)((rw + GF2_FT_WORDS - 1) / GF2_FT_WORDS)), dim3(256), 0, S.sA>>>(S.M, rows, S.srows, h->tw0, rw, d_rhs,
	                                                                                                     (int)np, rhs_stride, acc);
	k_put_rhs<<<dim3(gx), dim3(256), 0, S.sA>>>(acc, rows, cols, S.srows, S.M);
	const i64 nrw = ((cols & 63) + np + 63) / 64;
	k_check_rhs_many<<<dim3((unsigned)std::min<i64>(1024, gx), (unsigned)nrw), dim3(256), 0, S.sA>>>(S.M, rows, S.srows, cols, np, S.died, bad);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[2], S.sA));
	std::vector<int> yc((size_t)np);
	for (i64 j = 0; j < np; j++) yc[(size_t)j] = (int)(cols + j);
	BackSubScope scope{ S };
	int rc = enqueue_backsub(S, yc);
	if (rc) return rc;
	HIPCHK(hipEventRecord(ev[3], S.sA));
	std::vector<u64> hout((size_t)(np * cwx));
	u64 hbad = 0;
	HIPCHK(hipMemcpyAsync(hout.data(), S.bs.out, sizeof(u64) * hout.size(), hipMemcpyDeviceToHost, S.sA));
	HIPCHK(hipMemcpyAsync(&hbad, bad, sizeof(u64), hipMemcpyDeviceToHost, S.sA));
	HIPCHK(hipEventRecord(ev[4], S.sA));
	HIPCHK(hipStreamSynchronize(S.sA));
	float ms[4] = {0, 0, 0, 0};
	for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
	const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	for (i64 j = 0; j < np; j++) {
		const bool ok = !((hbad >> j) & 1);
		std::unique_ptr<gf2bv_result> R = new_result(ok, cols, h->piv.data(), h->rank, hout.data() + (size_t)(j * cwx));
		if (ok && h->mode == GF2BV_MODE_AFFINE_SPACE) R->basis = h->basis;
		gf2bv_stats &st = R->stats;
		st = h->fst;
		st.rank = R->rank; st.dimension = R->dim; st.status = R->status;
		st.ms_pack = ms[0]; st.ms_eliminate = ms[1]; st.ms_backsub = ms[2]; st.ms_export = ms[3]; st.ms_total = total;
		st.ms_sweep = 0;
		out[j] = R.release();
	}
	return GF2BV_OK;
}

int factor_solve(gf2bv_factor *h, const u64 *rhs, bool on_device, i64 nrhs, i64 rhs_words, hipStream_t stream, gf2bv_result **out)
{
	std::lock_guard<std::mutex> lk(h->mu);
	// (checked again under the lock: an append on another thread may have finished between check_factor_args and here)
	if (h->failed) return fail(GF2BV_ERR_ARG, kFailedHandle);
	if (rhs_words < h->rw) return fail(GF2BV_ERR_ARG, "rhs_words does not cover one bit per row");
	const auto t0 = std::chrono::steady_clock::now();
	Solver &S = h->S;
	S.kn.refresh();
	HIPCHK(hipSetDevice(h->device));
	const i64 rw = h->rw, C = kFactorSlots;
	Held held(h->device, S.sA);
	u64 *acc = nullptr, *bad = nullptr, *d = nullptr;
	HIPCHK(held.get((void **)&acc, sizeof(u64) * std::max<i64>(1, h->rows)));
	HIPCHK(held.get((void **)&bad, sizeof(u64)));
	if (!on_device) HIPCHK(held.get((void **)&d, sizeof(u64) * C * rw));
	hipEvent_t ev[5];
	for (hipEvent_t &e : ev) HIPCHK(held.event(&e));
	// Ordering contract: the right-hand sides are whatever `stream` (the caller's stream, NULL = the null stream) has produced
	// when this call is made.  S.sA is one of the library's own non-blocking streams, which is not ordered against any other
	// stream by itself: it waits for an event recorded on `stream` here.
	if (on_device) {
		HIPCHK(hipEventRecord(ev[0], stream));
		HIPCHK(hipStreamWaitEvent(S.sA, ev[0], 0));
	}
	std::vector<std::unique_ptr<gf2bv_result>> res((size_t)nrhs);
	std::vector<gf2bv_result *> part((size_t)C);
	for (i64 j0 = 0; j0 < nrhs; j0 += C) {
		const i64 np = std::min(C, nrhs - j0);
		HIPCHK(hipEventRecord(ev[0], S.sA));
		const u64 *src = rhs + j0 * rhs_words;
		i64 stride = rhs_words;
		if (!on_device) {             // (only the words that hold rows go up)
			HIPCHK(hipMemcpy2DAsync(d, rw * 8, src, rhs_words * 8, rw * 8, np, hipMemcpyHostToDevice, S.sA));
			src = d; stride = rw;
		}
		int rc = factor_pass(h, src, np, stride, ev, t0, acc, bad, part.data());
		if (rc) return rc;
		for (i64 j = 0; j < np; j++) res[(size_t)(j0 + j)].reset(part[(size_t)j]);
	}
	for (i64 j = 0; j < nrhs; j++) out[j] = res[(size_t)j].release();
	return GF2BV_OK;
}

int check_factor_args(const gf2bv_factor *h, const void *rhs, i64 nrhs, i64 rhs_words, gf2bv_result **out)
{
	if (!h || !out || !rhs) return fail(GF2BV_ERR_ARG, "null pointer");
	if (nrhs < 1) return fail(GF2BV_ERR_ARG, "nrhs must be at least 1");
	for (i64 j = 0; j < nrhs; j++) out[j] = nullptr;
	if (h->failed) return fail(GF2BV_ERR_ARG, "the handle is unusable: an append failed after it had started to change it");
	if (rhs_words < h->rw) return fail(GF2BV_ERR_ARG, "rhs_words does not cover one bit per row");
	return GF2BV_OK;
}

// ---- equations appended to a kept factorization (gf2bv_factor_append_*) -----------------------------------------------------
// Appending k rows B keeps every result equal to a fresh factorization of the stacked matrix: the pivots of [A; B] are the column
// rank profile, a superset of A's, and with the pivot set fixed the origin and the kernel basis are unique.  So the kept U stays,
// and the new rows only have to be reduced by it and eliminated among themselves:
//   grow    M is re-tiled into slabs with room for the new rows and T columns for them (capacity in whole kAppendRound rows, so
//           that small appends mostly find room), B is packed below the kept rows, each new row gets its identity bit in T;
//   reduce  word by word (the words with pivots, ascending), B ^= (B's bits at the word's pivot columns) x (those pivot rows),
//           one launch per word over the tiles from that word on (k_append_reduce): B ends zero at every old pivot column;
//   new     B's bits at the old free columns gathered (k_append_gather), Gauss-Jordan on those in column order with the row
//           operations recorded (k_append_eliminate, one workgroup), applied to the whole rows, T included (k_append_combine);
//   merge   old pivot rows of a word that gained pivots reduced by the new ones (k_append_backreduce: the back-substitution
//           takes the pivot rows of a word as mutually reduced), the pivot lists and panel records rebuilt on the host and
//           uploaded, new pivot rows retired in `died` (rows without a pivot stay alive: the consistency check reads them);
//           mode 1 recomputes the kernel basis with one back-substitution, as factor_matrix does.
// Rows go through reduce / new / merge in chunks of kAppendChunk (one workgroup eliminates a chunk); a later chunk sees the
// pivots of the earlier ones, exactly as appending them one after the other would.
constexpr i64 kAppendChunk = 1024, kAppendRound = 1024;

// Everything an append allocates, taken before the kept state is changed (a refusal there leaves the handle as it was): the
// reduction's snapshots, the gathered rows, the free columns, the elimination's output, the merge's item and pivot lists.
struct AppendBufs {
	u64 *snap = nullptr, *W = nullptr;
	int *fc = nullptr, *out = nullptr, *nb = nullptr, *nr = nullptr, *drow = nullptr, *dval = nullptr;
	int4 *items = nullptr;
	hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
};

int check_append_args(const gf2bv_factor *h, const MatrixInput &in, i64 k)
{
	if (!h) return fail(GF2BV_ERR_ARG, "null pointer");
	if (h->failed) return fail(GF2BV_ERR_ARG, kFailedHandle);
	if (k < 1) return fail(GF2BV_ERR_ARG, "rows must be at least 1");
	if (h->rows + k >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, "system too large");
	return check_matrix_form(in, k, h->cols);
}

// the merged pivot lists of the handle (old pivots + new ones: column, physical row) -> host copies and device arrays
int append_merge(gf2bv_factor *h, const std::vector<std::pair<int, int>> &add, const AppendBufs &B)
{
	Solver &S = h->S;
	const int np = S.npanels;
	std::vector<std::pair<int, int>> all;
	all.reserve(h->piv.size() + add.size());
	for (size_t i = 0; i < h->piv.size(); i++) all.emplace_back(h->piv[i], h->urow[i]);
	all.insert(all.end(), add.begin(), add.end());
	std::sort(all.begin(), all.end());
	// old pivot rows of the words that gained pivots: reduced by the new pivot rows of their word
	std::vector<int> nbit(add.size()), nrow(add.size());
	std::vector<int4> items;
	{
		std::vector<std::pair<int, int>> na(add);
		std::sort(na.begin(), na.end());
		for (size_t j = 0; j < na.size(); j++) { nbit[j] = na[j].first & 63; nrow[j] = na[j].second; }
		for (size_t j0 = 0; j0 < na.size();) {
			const int w = na[j0].first >> 6;
			size_t j1 = j0;
			while (j1 < na.size() && (na[j1].first >> 6) == w) j1++;
			const PanelRec &rec = h->hp[(size_t)w];
			for (int r = 0; r < rec.p; r++)
				items.push_back(make_int4(h->urow[(size_t)(rec.start + r)], w, ((h->piv[(size_t)(rec.start + r)] & 63) << 8) | (int)(j1 - j0), (int)j0));
			j0 = j1;
		}
	}
	const i64 rank = (i64)all.size();
	std::vector<PanelRec> hp((size_t)np);
	for (auto &r : hp) { r.start = 0; r.p = 0; r.mask = 0; }
	std::vector<int32_t> piv((size_t)rank), urow((size_t)rank);
	for (i64 i = 0; i < rank; i++) {
		piv[(size_t)i] = all[(size_t)i].first; urow[(size_t)i] = all[(size_t)i].second;
		PanelRec &r = hp[(size_t)(all[(size_t)i].first >> 6)];
		r.p++; r.mask |= 1ull << (all[(size_t)i].first & 63);
	}
	for (int w = 0, st = 0; w < np; w++) { hp[(size_t)w].start = st; st += hp[(size_t)w].p; }
	// (items: old pivot rows, at most cols of them; new pivots: at most kAppendChunk -- the sizes of B's arrays)
	if (!items.empty()) {
		HIPCHK(hipMemcpyAsync(B.items, items.data(), sizeof(int4) * items.size(), hipMemcpyHostToDevice, S.sA));
		HIPCHK(hipMemcpyAsync(B.nb, nbit.data(), sizeof(int) * nbit.size(), hipMemcpyHostToDevice, S.sA));
		HIPCHK(hipMemcpyAsync(B.nr, nrow.data(), sizeof(int) * nrow.size(), hipMemcpyHostToDevice, S.sA));
		k_append_backreduce<<<dim3((unsigned)items.size()), dim3(256), 0, S.sA>>>(S.M, S.srows, S.ntiles, B.items, B.nb, B.nr);
		HIPCHK(hipGetLastError());
	}
	std::vector<int> drow(add.size()), dval(add.size());
	for (size_t j = 0; j < add.size(); j++) { drow[j] = add[j].second; dval[j] = add[j].first >> 6; }    // (not GF2_NEVER: a pivot row)
	HIPCHK(hipMemcpyAsync(S.panels, hp.data(), sizeof(PanelRec) * np, hipMemcpyHostToDevice, S.sA));
	if (rank) HIPCHK(hipMemcpyAsync(S.pivcol, piv.data(), sizeof(int) * rank, hipMemcpyHostToDevice, S.sA));
	if (rank) HIPCHK(hipMemcpyAsync(S.urow, urow.data(), sizeof(int) * rank, hipMemcpyHostToDevice, S.sA));
	const int rank32 = (int)rank;
	HIPCHK(hipMemcpyAsync(&S.st->rank, &rank32, sizeof(int), hipMemcpyHostToDevice, S.sA));
	HIPCHK(hipMemcpyAsync(B.drow, drow.data(), sizeof(int) * drow.size(), hipMemcpyHostToDevice, S.sA));
	HIPCHK(hipMemcpyAsync(B.dval, dval.data(), sizeof(int) * dval.size(), hipMemcpyHostToDevice, S.sA));
	k_append_died<<<dim3((unsigned)((add.size() + 255) / 256)), dim3(256), 0, S.sA>>>(S.died, B.drow, B.dval, (int)add.size());
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(S.sA));          // (the host sources above live on this frame)
	h->hp = std::move(hp); h->piv = std::move(piv); h->urow = std::move(urow); h->rank = rank;
	return GF2BV_OK;
}

// rows r0 .. r0 + k of M (packed, identity bits set; k <= kAppendChunk) reduced by the kept pivots, eliminated among themselves
// and merged in
int append_chunk(gf2bv_factor *h, i64 r0, i64 k, const AppendBufs &B, double ms[3])
{
	Solver &S = h->S;
	const i64 cols = h->cols, ntiles = S.ntiles, srows = S.srows;
	const hipEvent_t *ev = B.ev;
	u64 *snap = B.snap, *W = B.W;
	int *fc_d = B.fc, *out_d = B.out;
	HIPCHK(hipEventRecord(ev[0], S.sA));
	// reduce: the words with pivots in turn
	std::vector<int> pw;
	for (int w = 0; w < S.npanels; w++) if (h->hp[(size_t)w].p) pw.push_back(w);
	const unsigned gk = (unsigned)((k + 255) / 256);
	if (!pw.empty()) k_append_snap<<<dim3(gk), dim3(256), 0, S.sA>>>(S.M, srows, r0, k, pw[0], snap);
	for (size_t j = 0; j < pw.size(); j++) {
		const i64 w = pw[j], wn = j + 1 < pw.size() ? pw[j + 1] : -1;
		const i64 nt = ntiles - (w >> 1);
		k_append_reduce<<<dim3((unsigned)((nt + 3) / 4), (unsigned)((k + 63) / 64)), dim3(256), 0, S.sA>>>(
			S.M, srows, r0, k, w, wn, ntiles, S.panels, S.urow, S.pivcol, snap + (j & 1) * kAppendChunk, snap + ((j + 1) & 1) * kAppendChunk);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[1], S.sA));
	// new pivots among the reduced rows, at the free columns
	std::vector<int> fc;
	{
		std::vector<char> isp((size_t)cols, 0);
		for (int32_t c : h->piv) isp[(size_t)c] = 1;
		for (i64 c = 0; c < cols; c++) if (!isp[(size_t)c]) fc.push_back((int)c);
	}
	const i64 nf = (i64)fc.size(), nfw = (nf + 63) / 64, kw = (k + 63) / 64, ldw = nfw + kw;
	std::vector<std::pair<int, int>> add;
	if (nf) {
		HIPCHK(hipMemcpyAsync(fc_d, fc.data(), sizeof(int) * nf, hipMemcpyHostToDevice, S.sA));
		k_append_gather<<<dim3((unsigned)((k * ldw + 255) / 256)), dim3(256), 0, S.sA>>>(S.M, srows, r0, k, fc_d, nf, nfw, ldw, W);
		k_append_eliminate<<<dim3(1), dim3(1024), 0, S.sA>>>(W, (int)k, nfw, ldw, out_d, out_d + kAppendChunk, out_d + 2 * kAppendChunk);
		k_append_combine<<<dim3((unsigned)std::min<i64>(ntiles, 2048)), dim3(256), 0, S.sA>>>(S.M, srows, r0, (int)k, ntiles, W, nfw, ldw);
		HIPCHK(hipGetLastError());
		std::vector<int> out((size_t)(2 * kAppendChunk + 1));
		HIPCHK(hipMemcpyAsync(out.data(), out_d, sizeof(int) * out.size(), hipMemcpyDeviceToHost, S.sA));
		HIPCHK(hipStreamSynchronize(S.sA));      // (fc and out live on this frame)
		const int n = out[2 * kAppendChunk];
		for (int j = 0; j < n; j++) add.emplace_back(fc[(size_t)out[(size_t)j]], (int)(r0 + out[(size_t)(kAppendChunk + j)]));
	}
	HIPCHK(hipEventRecord(ev[2], S.sA));
	if (!add.empty()) {
		int rc = append_merge(h, add, B);
		if (rc) return rc;
	}
	HIPCHK(hipEventRecord(ev[3], S.sA));
	HIPCHK(hipStreamSynchronize(S.sA));
	for (int i = 0; i < 3; i++) { float t = 0; (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]); ms[i] += t; }
	return GF2BV_OK;
}

int factor_append(gf2bv_factor *h, const MatrixInput &in, i64 k, hipStream_t stream)
{
	std::lock_guard<std::mutex> lk(h->mu);
	if (h->failed) return fail(GF2BV_ERR_ARG, kFailedHandle);      // (again under the lock, as factor_solve does)
	Solver &S = h->S;
	S.kn.refresh();
	HIPCHK(hipSetDevice(h->device));
	const i64 rows = h->rows, cols = h->cols, rows2 = rows + k, rw2 = (rows2 + 63) / 64;
	const bool grow = rows2 > h->cap_rows;
	const i64 cap = grow ? round_up(rows2, kAppendRound) : h->cap_rows;
	const i64 srows2 = grow ? slab_rows(cap) : S.srows, ntiles2 = grow ? tiles_for(h->tw0 + (cap + 63) / 64) : S.ntiles;
	double ms[5] = {0, 0, 0, 0, 0};
	// everything the append allocates is taken before the handle is touched: an argument error or a refusal leaves it as it was
	u64 *M2 = S.M;
	int *died2 = S.died;
	if (grow) {
		M2 = nullptr; died2 = nullptr;
		const char *nomem = "the grown factorization does not fit on the device";
		if (int rc = alloc_or_nomem((void **)&M2, sizeof(u64) * ntiles2 * TW * srows2 + kOuterSlackBytes, h->device, nomem, "grown working matrix")) return rc;
		if (int rc = alloc_or_nomem((void **)&died2, sizeof(int) * cap, h->device, nomem, "grown row records")) { pool().release(M2); return rc; }
	}
	// (on an error past this point the grown buffers go back to the pool; the kept state is only replaced at the end)
	struct Grown {
		u64 *M; int *died; bool own;
		~Grown() { if (own) { pool().release(M); pool().release(died); } }
	} grown{ M2, died2, grow };
	Held held(h->device, S.sA);             // (declared after `grown`: the stream is waited for before the grown buffers go back)
	const i64 kc = std::min(k, kAppendChunk);
	const i64 nfw = (cols + 63) / 64, ldw = nfw + (kc + 63) / 64;
	AppendBufs B;
	HIPCHK(held.get((void **)&B.snap, sizeof(u64) * 2 * kAppendChunk));
	HIPCHK(held.get((void **)&B.W, sizeof(u64) * kc * ldw));
	HIPCHK(held.get((void **)&B.fc, sizeof(int) * cols));
	HIPCHK(held.get((void **)&B.out, sizeof(int) * (2 * kAppendChunk + 1)));
	HIPCHK(held.get((void **)&B.items, sizeof(int4) * cols));
	for (int **p : { &B.nb, &B.nr, &B.drow, &B.dval }) HIPCHK(held.get((void **)p, sizeof(int) * kAppendChunk));
	for (hipEvent_t &e : B.ev) HIPCHK(held.event(&e));
	hipEvent_t g0, g1;
	HIPCHK(held.event(&g0)); HIPCHK(held.event(&g1));
	// Ordering contract: the appended rows are whatever `stream` (the caller's stream, NULL = the null stream) has produced when
	// this call is made.  S.sA is one of the library's own non-blocking streams, which is not ordered against any other stream by
	// itself: it waits for an event recorded on `stream` here.
	if (in.d_words) {
		HIPCHK(hipEventRecord(g0, stream));
		HIPCHK(hipStreamWaitEvent(S.sA, g0, 0));
	}
	HIPCHK(hipEventRecord(g0, S.sA));
	if (grow) {
		k_append_retile<<<dim3((unsigned)((srows2 + 255) / 256), (unsigned)std::min<i64>(ntiles2, 64)), dim3(256), 0, S.sA>>>(
			S.M, S.srows, rows, S.ntiles, M2, srows2, ntiles2);
		HIPCHK(hipMemcpyAsync(died2, S.died, sizeof(int) * rows, hipMemcpyDeviceToDevice, S.sA));
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipMemsetAsync(died2 + rows, GF2_NEVER & 0xff, sizeof(int) * k, S.sA));
	if (int rc = pack_coefficients(in, k, cols, ntiles2, srows2, S.sA, held, M2 + rows * TW)) return rc;
	k_append_init<<<dim3((unsigned)((k + 255) / 256), (unsigned)std::min<i64>(h->tw0 + rw2 - (cols >> 6), 64)), dim3(256), 0, S.sA>>>(
		rows, k, cols, srows2, h->tw0, h->tw0 + rw2, M2);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(g1, S.sA));
	HIPCHK(hipStreamSynchronize(S.sA));
	{ float t = 0; (void)hipEventElapsedTime(&t, g0, g1); ms[0] = t; }
	// the kept state changes from here on: a failure past this point leaves the handle marked unusable (h->failed)
	if (grow) {
		pool().release(S.M);
		S.M = M2;
		if (h->died_buf) pool().release(h->died_buf);
		h->died_buf = died2;
		S.died = died2;
		grown.own = false;
		h->cap_rows = cap;
		S.srows = srows2; S.ntiles = ntiles2; S.m_stride = ntiles2 * TW * srows2;
	}
	auto rest = [&]() -> int {
		for (i64 c0 = 0; c0 < k; c0 += kAppendChunk) {
			int rc = append_chunk(h, rows + c0, std::min(kAppendChunk, k - c0), B, ms + 1);
			if (rc) return rc;
		}
		std::vector<u64> basis;
		if (h->mode == GF2BV_MODE_AFFINE_SPACE) {
			const auto tb = std::chrono::steady_clock::now();
			if (int rc = factor_basis(h, basis)) return rc;
			ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
		}
		h->basis = std::move(basis);
		h->rows = rows2; h->rw = rw2;
		S.rows = rows2; S.wt = h->tw0 + rw2; S.nrhs = (int)(S.wt * 64 - cols);
		h->fst.rows = rows2; h->fst.stride_words = S.wt; h->fst.rank = h->rank; h->fst.dimension = cols - h->rank;
		h->device_bytes = factor_device_bytes(h);
		return GF2BV_OK;
	};
	if (int rc = rest()) {
		h->failed = true;
		const std::string why = g_err;
		return fail(GF2BV_ERR_HIP, (std::string(kFailedHandle) + ": " + why).c_str());
	}
	if (S.kn.trace)       // times of the append's phases
		fprintf(stderr, "[gf2bv trace] append %lld rows: grow %.3f reduce %.3f new %.3f merge %.3f basis %.3f ms\n", (long long)k, ms[0], ms[1], ms[2], ms[3], ms[4]);
	return GF2BV_OK;
}

// An independent handle: the host fields and the solver's plan as they are, the kept state copied device to device into resources of
// the copy's own: a stream, four timing events, the matrix, an arena and, where the original has one, a died_buf.  Nothing is borrowed.
int factor_copy(gf2bv_factor *h, gf2bv_factor **out)
{
	std::lock_guard<std::mutex> lk(h->mu);
	const Solver &S = h->S;
	HIPCHK(hipSetDevice(h->device));
	std::unique_ptr<gf2bv_factor> c(new gf2bv_factor());
	c->rows = h->rows; c->cols = h->cols; c->tw0 = h->tw0; c->rw = h->rw; c->cw = h->cw;
	c->mode = h->mode; c->device = h->device; c->rank = h->rank;
	c->piv = h->piv; c->basis = h->basis; c->fst = h->fst; c->device_bytes = h->device_bytes;
	c->cap_rows = h->cap_rows; c->hp = h->hp; c->urow = h->urow;
	Solver &D = c->S;
	D.plan() = S.plan();
	HIPCHK(pool().stream(&D.sA, h->device, false));
	D.own_sA = true;
	for (hipEvent_t *e : { &D.ev0, &D.ev1, &D.ev2, &D.ev3 }) HIPCHK(pool().event(e, true));
	const char *nomem = "the copy of the factorization does not fit on the device";
	int rc = alloc_or_nomem((void **)&D.M, sizeof(u64) * S.ntiles * TW * S.srows + kOuterSlackBytes, h->device, nomem, "working matrix");
	if (!rc) rc = alloc_or_nomem(&D.arena, S.lay.stride, h->device, nomem, "arena");
	if (!rc && h->died_buf) rc = alloc_or_nomem((void **)&c->died_buf, sizeof(int) * h->cap_rows, h->device, nomem, "row records");
	if (rc) return rc;
	D.bind(D.lay, D.arena, D.kn.pc);
	if (c->died_buf) D.died = c->died_buf;
	// the copy starts after what the original's stream has queued
	HIPCHK(hipStreamSynchronize(S.sA));
	HIPCHK(hipMemcpyAsync(D.M, S.M, sizeof(u64) * S.ntiles * TW * S.srows, hipMemcpyDeviceToDevice, D.sA));
	HIPCHK(hipMemcpyAsync(D.arena, S.arena, S.lay.stride, hipMemcpyDeviceToDevice, D.sA));
	if (h->died_buf) HIPCHK(hipMemcpyAsync(c->died_buf, h->died_buf, sizeof(int) * h->cap_rows, hipMemcpyDeviceToDevice, D.sA));
	HIPCHK(hipStreamSynchronize(D.sA));
	*out = c.release();
	return GF2BV_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int gf2bv_version(void) { return 100; }

// sha256 (first 16 hex digits) over gf2_solver.hip + gf2_kernels.hip.h + gf2bv_hip.h, handed in by gf2bv_amd/build.py; the
// marker in front lets build.py read the id of an existing library without loading it (staleness by content, not by mtime)
#ifndef GF2BV_BUILD_ID
#define GF2BV_BUILD_ID "unknown"
#endif
static const char g_build_id[] = "GF2BV_BUILD_ID=" GF2BV_BUILD_ID;
const char *gf2bv_build_id(void) { return g_build_id + 15; }

int gf2bv_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

const char *gf2bv_last_error(void) { return g_err.c_str(); }

int gf2bv_solve_device(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words, int mode,
                       int device, void *stream, int time_kernels, gf2bv_result **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	MatrixInput in; in.d_words = (const u64 *)d_aug; in.stride = stride_words;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	if (const Knobs kn = Knobs::read(Knobs::kSmall); small_eligible(kn, rows, cols) && !time_kernels) return small_solve(kn, in, rows, cols, mode, device, (hipStream_t)stream, out);
	Solver S;
	S.t_begin = std::chrono::steady_clock::now();
	S.device = device;
	S.sA = (hipStream_t)stream;
	S.src = (const u64 *)d_aug;
	S.rows = rows; S.cols = cols; S.stride = stride_words; S.mode = mode;
	S.time_kernels = time_kernels != 0;
	rc = solver_enqueue(S);
	if (rc) return rc;
	return solver_finish(S, out);
	});
}

int gf2bv_solve_batch_device(void *d_aug, int64_t nsys, int64_t sys_stride_words, int64_t rows, int64_t cols,
                             int64_t stride_words, int mode, int device, void *stream, int time_kernels, gf2bv_result **out)
{
	return guarded([&]() -> int {
	if (!out || nsys < 0) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 s = 0; s < nsys; s++) out[s] = nullptr;
	MatrixInput in; in.d_words = (const u64 *)d_aug; in.stride = stride_words;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (rc) return rc;
	if ((sys_stride_words & 1) || sys_stride_words < rows * stride_words)
		return fail(GF2BV_ERR_ARG, "sys_stride_words must be even and at least rows * stride_words");
	rc = check_device(device);
	if (rc) return rc;
	// Independent systems of one shape run as GANGS: the forward elimination of `gang` systems is one set
	// of launches (blockIdx.y = system), so the latency-bound panel path and the host's ~3500 launches
	// per elimination are shared by the whole gang and the bulk updates of all its systems fill the chip.
	const Knobs kn = Knobs::read();
	const i64 gang = pick_gang(kn, nsys, rows, cols);
	// Ordering contract: the matrices are whatever `stream` (the caller's stream, NULL = the null stream) has
	// produced when this call is made.  The gangs run on the library's own non-blocking streams, which are not
	// ordered against any other stream by themselves: each waits for an event recorded on `stream` here.
	Held held(device);
	hipEvent_t ready = nullptr;
	HIPCHK(held.event(&ready, false));
	HIPCHK(hipEventRecord(ready, (hipStream_t)stream));
	return run_gangs(kn, device, nsys, gang, ready, 0, out, [&](Solver &S, i64 s0, int, void *) -> int {
		S.src = (const u64 *)d_aug + s0 * sys_stride_words;
		S.src_sys_words = sys_stride_words;
		S.rows = rows; S.cols = cols; S.stride = stride_words; S.mode = mode;
		S.time_kernels = time_kernels != 0;
		return GF2BV_OK;
	});
	});
}

int gf2bv_solve_words(const uint64_t *aug, int64_t rows, int64_t cols, int64_t stride_words, int mode,
                      int device, gf2bv_result **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	MatrixInput in; in.h_words = reinterpret_cast<const u64 *>(aug); in.stride = stride_words;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	if (const Knobs kn = Knobs::read(Knobs::kSmall); small_eligible(kn, rows, cols)) return small_solve(kn, in, rows, cols, mode, device, nullptr, out);
	const i64 wt = (cols + 1 + 63) / 64;
	Solver S;
	S.t_begin = std::chrono::steady_clock::now();
	S.device = device;
	HIPCHK(pool().stream(&S.sA, device, false));
	S.own_sA = true;
	S.rows = rows; S.cols = cols; S.mode = mode;
	S.stride = wt;
	HIPCHK(pool().alloc((void **)&S.tmp_src, sizeof(u64) * std::max<i64>(1, rows) * S.stride, device));
	S.src = S.tmp_src;
	Held held(device, S.sA);                // (declared after S: what the entry holds goes back before what the solver owns)
	hipEvent_t p0, p1;
	HIPCHK(held.event(&p0)); HIPCHK(held.event(&p1));
	HIPCHK(hipEventRecord(p0, S.sA));
	if (rows > 0)
		HIPCHK(hipMemcpy2DAsync(S.tmp_src, S.stride * 8, aug, stride_words * 8, wt * 8, rows, hipMemcpyHostToDevice, S.sA));
	// bits above column `cols` are ignored by the reference (_internal.c:414): they are never
	// pivot candidates (colmask), never exported, and the RHS is read at exactly column `cols`.
	HIPCHK(hipEventRecord(p1, S.sA));
	rc = solver_enqueue(S);
	if (rc == GF2BV_OK) {
		(void)hipEventSynchronize(p1);
		(void)hipEventElapsedTime(&S.ms_pack, p0, p1);
		rc = solver_finish(S, out);
	}
	return rc;
	});
}

// digit_off[] holds ABSOLUTE digit positions (a share of a larger batch, from gf2bv_solve_batch_digits_multi, does not start
// at 0): only digits[digit_off[0] .. digit_off[nsys * rows]) are uploaded and the pack kernel sees them through a rebased pointer.
int gf2bv_solve_batch_digits(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit, int64_t nsys,
                             int64_t rows, int64_t cols, int mode, int device, gf2bv_result **out)
{
	return guarded([&]() -> int {
	int rc = check_digits_batch(digits, digit_off, bits_per_digit, nsys, rows, cols, mode, out);
	if (rc) return rc;
	rc = check_device(device);
	if (rc) return rc;
	if (nsys == 0) return GF2BV_OK;
	const i64 wt = (cols + 1 + 63) / 64, ntiles = tiles_for(wt), srows = slab_rows(rows);
	const i64 m_stride = ntiles * TW * srows;
	const i64 nrows_all = nsys * rows;
	// The offsets go up once; the DIGITS go up gang by gang, each on the stream of the host thread that takes the gang (round 5: two
	// threads, as in gf2bv_solve_batch_device -- one gang's upload and pack run under the other's elimination, and two latency-bound
	// gangs of sparse systems overlap; before: one upload of everything, then the gangs one after the other on one stream -- 16 MT19937
	// recovery systems 43 ms, 15 of them the upload).  Every gang packs its own systems straight into tile-major slabs.
	Held G(device);
	i64 *d_off = nullptr;
	hipEvent_t ready = nullptr;
	HIPCHK(G.stream(2));
	HIPCHK(G.get((void **)&d_off, sizeof(i64) * (nrows_all + 1)));
	HIPCHK(hipMemcpyAsync(d_off, digit_off, sizeof(i64) * (nrows_all + 1), hipMemcpyHostToDevice, G.st));
	HIPCHK(G.event(&ready, false));
	HIPCHK(hipEventRecord(ready, G.st));
	const Knobs kn = Knobs::read();
	const i64 gang = pick_gang(kn, nsys, rows, cols);
	const i64 ngangs = (nsys + gang - 1) / gang;
	i64 max_dig = 1;
	for (i64 q = 0; q < ngangs; q++)
		max_dig = std::max<i64>(max_dig, digit_off[std::min<i64>(nsys, (q + 1) * gang) * rows] - digit_off[q * gang * rows]);
	return run_gangs(kn, device, nsys, gang, ready, sizeof(uint32_t) * max_dig, out, [&](Solver &S, i64 s0, int ns, void *buf) -> int {
		uint32_t *dig = (uint32_t *)buf;
		const i64 d0 = digit_off[s0 * rows], nd = digit_off[(s0 + ns) * rows] - d0;
		if (nd) HIPCHK(hipMemcpyAsync(dig, digits + d0, sizeof(uint32_t) * nd, hipMemcpyHostToDevice, S.sA));
		S.rows = rows; S.cols = cols; S.mode = mode;
		S.stride = ntiles * TW;
		HIPCHK(pool().alloc((void **)&S.M, sizeof(u64) * m_stride * S.nsys + kOuterSlackBytes, device));
		if (rows * ntiles * TW > 0)
			k_pack_digits<<<dim3((unsigned)((ntiles * TW + 255) / 256), (unsigned)std::min<i64>(rows, 65535), S.nsys), dim3(256), 0, S.sA>>>(
				dig, d_off + s0 * rows, bits_per_digit, (i64)rows, (i64)cols, ntiles * TW, srows, S.M, SysStride{m_stride, 0}, d0);
		HIPCHK(hipGetLastError());
		return GF2BV_OK;
	});
	});
}

// The same batch over SEVERAL devices (the reference solves one system per m4ri_solve call on one core; independent
// systems -- one per output bit / per instance in the recovery examples -- are this path's natural shard unit):
// entry k of devices[] takes the k-th contiguous share of the systems on its own host thread (a device may be listed more
// than once: its shares then run as concurrent gangs on it), results land in out[] in input order.  No collective and no
// torch: one process drives every GPU of the node.
int gf2bv_solve_batch_digits_multi(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit, int64_t nsys,
                                   int64_t rows, int64_t cols, int mode, const int *devices, int ndevices,
                                   gf2bv_result **out)
{
	return guarded([&]() -> int {
	int rc = check_digits_batch(digits, digit_off, bits_per_digit, nsys, rows, cols, mode, out);
	if (rc) return rc;
	if (!devices || ndevices < 1) return fail(GF2BV_ERR_ARG, "null pointer");
	for (int k = 0; k < ndevices; k++) { rc = check_device(devices[k]); if (rc) return rc; }
	const int nshares = (int)std::min<i64>(ndevices, std::max<i64>(nsys, 1));
	rc = run_on_threads(nshares, [&](int k) {
		const i64 lo = nsys * k / nshares, hi = nsys * (k + 1) / nshares;
		return gf2bv_solve_batch_digits(digits, digit_off + lo * rows, bits_per_digit, hi - lo, rows, cols, mode, devices[k], out + lo);
	});
	if (rc) for (i64 s = 0; s < nsys; s++) { delete out[s]; out[s] = nullptr; }
	return rc;
	});
}

int gf2bv_solve_digits(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit, int64_t rows,
                       int64_t cols, int mode, int device, gf2bv_result **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	MatrixInput in; in.h_digits = digits; in.h_off = reinterpret_cast<const i64 *>(digit_off); in.bpd = bits_per_digit;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	if (const Knobs kn = Knobs::read(Knobs::kSmall); small_eligible(kn, rows, cols)) return small_solve(kn, in, rows, cols, mode, device, nullptr, out);
	Solver S;
	S.t_begin = std::chrono::steady_clock::now();
	S.device = device;
	HIPCHK(pool().stream(&S.sA, device, false));
	S.own_sA = true;
	S.rows = rows; S.cols = cols; S.mode = mode;
	const i64 ntiles = tiles_for((cols + 1 + 63) / 64), srows = slab_rows(rows);
	S.stride = ntiles * TW;
	HIPCHK(pool().alloc((void **)&S.M, sizeof(u64) * ntiles * TW * srows + kOuterSlackBytes, device));     // packed straight into tiles
	Held held(device, S.sA);                // digits, offsets and the pack events go back to the pool on every path
	hipEvent_t p0, p1;
	HIPCHK(held.event(&p0)); HIPCHK(held.event(&p1));
	HIPCHK(hipEventRecord(p0, S.sA));
	if ((rc = pack_coefficients(in, rows, cols, ntiles, srows, S.sA, held, S.M))) return rc;
	HIPCHK(hipEventRecord(p1, S.sA));
	rc = solver_enqueue(S);
	if (rc == GF2BV_OK) {
		(void)hipEventSynchronize(p1);
		(void)hipEventElapsedTime(&S.ms_pack, p0, p1);
		rc = solver_finish(S, out);
	}
	return rc;
	});
}

// Many right-hand sides of one matrix (_internal.c:398-455: the reference factors A alone, then solves against B): see solve_rhs.
int gf2bv_solve_rhs_digits(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit, int64_t rows, int64_t cols,
                           const uint64_t *rhs, int64_t nrhs, int64_t rhs_words, int mode, int device, gf2bv_result **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 j = 0; j < nrhs; j++) out[j] = nullptr;
	MatrixInput in; in.h_digits = digits; in.h_off = reinterpret_cast<const i64 *>(digit_off); in.bpd = bits_per_digit;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_rhs_args(rows, cols, rhs, false, nrhs, rhs_words);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	return solve_rhs(in, reinterpret_cast<const u64 *>(rhs), false, nrhs, rhs_words, rows, cols, mode, device, nullptr, false, out);
	});
}

int gf2bv_solve_rhs_words(const uint64_t *aug, int64_t rows, int64_t cols, int64_t stride_words,
                          const uint64_t *rhs, int64_t nrhs, int64_t rhs_words, int mode, int device, gf2bv_result **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 j = 0; j < nrhs; j++) out[j] = nullptr;
	MatrixInput in; in.h_words = reinterpret_cast<const u64 *>(aug); in.stride = stride_words;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_rhs_args(rows, cols, rhs, false, nrhs, rhs_words);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	return solve_rhs(in, reinterpret_cast<const u64 *>(rhs), false, nrhs, rhs_words, rows, cols, mode, device, nullptr, false, out);
	});
}

int gf2bv_solve_rhs_device(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words, const void *d_rhs, int64_t nrhs,
                           int64_t rhs_words, int mode, int device, void *stream, int time_kernels, gf2bv_result **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 j = 0; j < nrhs; j++) out[j] = nullptr;
	MatrixInput in; in.d_words = (const u64 *)d_aug; in.stride = stride_words;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_rhs_args(rows, cols, d_rhs, true, nrhs, rhs_words);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	return solve_rhs(in, (const u64 *)d_rhs, true, nrhs, rhs_words, rows, cols, mode, device, (hipStream_t)stream, time_kernels != 0, out);
	});
}

// A kept factorization (_internal.c:431-447: _mzd_pluq on A, then _mzd_pluq_solve_left on B, as two steps): see factor_matrix.
int gf2bv_factor_digits(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit, int64_t rows, int64_t cols, int mode,
                        int device, gf2bv_factor **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	MatrixInput in; in.h_digits = digits; in.h_off = reinterpret_cast<const i64 *>(digit_off); in.bpd = bits_per_digit;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	return factor_matrix(in, rows, cols, mode, device, nullptr, out);
	});
}

int gf2bv_factor_words(const uint64_t *aug, int64_t rows, int64_t cols, int64_t stride_words, int mode, int device, gf2bv_factor **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	MatrixInput in; in.h_words = reinterpret_cast<const u64 *>(aug); in.stride = stride_words;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	return factor_matrix(in, rows, cols, mode, device, nullptr, out);
	});
}

int gf2bv_factor_device(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words, int mode, int device, void *stream,
                        gf2bv_factor **out)
{
	return guarded([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	MatrixInput in; in.d_words = (const u64 *)d_aug; in.stride = stride_words;
	int rc = check_matrix_input(in, rows, cols, mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	return factor_matrix(in, rows, cols, mode, device, (hipStream_t)stream, out);
	});
}

int gf2bv_factor_solve(gf2bv_factor *h, const uint64_t *rhs, int64_t nrhs, int64_t rhs_words, gf2bv_result **out)
{
	return guarded([&]() -> int {
	int rc = check_factor_args(h, rhs, nrhs, rhs_words, out);
	if (rc) return rc;
	if ((rc = check_device(h->device))) return rc;
	return factor_solve(h, reinterpret_cast<const u64 *>(rhs), false, nrhs, rhs_words, nullptr, out);
	});
}

int gf2bv_factor_solve_device(gf2bv_factor *h, const void *d_rhs, int64_t nrhs, int64_t rhs_words, void *stream, int time_kernels,
                              gf2bv_result **out)
{
	(void)time_kernels;               // (a solve's phase times come from events either way)
	return guarded([&]() -> int {
	int rc = check_factor_args(h, d_rhs, nrhs, rhs_words, out);
	if (rc) return rc;
	if ((uintptr_t)d_rhs & 7) return fail(GF2BV_ERR_ARG, "the right-hand sides need 8-byte alignment");
	if ((rc = check_device(h->device))) return rc;
	return factor_solve(h, (const u64 *)d_rhs, true, nrhs, rhs_words, (hipStream_t)stream, out);
	});
}

// The getters take the handle's mutex like every other call: an append on another thread replaces rank, rows, piv and device_bytes.
int64_t gf2bv_factor_rank(const gf2bv_factor *h)
{
	if (!h) return -1;
	std::lock_guard<std::mutex> lk(h->mu);
	return !h->failed ? h->rank : -1;
}
// One locked copy: the entries written are one state of the handle.  Their number can only be known together with them (an append
// may raise the rank between two calls), so `o` has room for cols entries and the caller pre-fills it to count what was written.
int gf2bv_factor_pivots(const gf2bv_factor *h, int32_t *o)
{
	if (!h || !o) return fail(GF2BV_ERR_ARG, "null pointer");
	std::lock_guard<std::mutex> lk(h->mu);
	if (h->failed) return fail(GF2BV_ERR_ARG, kFailedHandle);
	if (!h->piv.empty()) memcpy(o, h->piv.data(), sizeof(int32_t) * h->piv.size());
	return GF2BV_OK;
}
int64_t gf2bv_factor_device_bytes(const gf2bv_factor *h)
{
	if (!h) return -1;
	std::lock_guard<std::mutex> lk(h->mu);
	return h->device_bytes;
}
void gf2bv_factor_free(gf2bv_factor *h)
{
	if (!h) return;
	{ std::lock_guard<std::mutex> lk(h->mu); }      // (a call still running on another thread finishes first)
	delete h;
}

// Equations appended to a kept factorization: see factor_append
int gf2bv_factor_append_words(gf2bv_factor *h, const uint64_t *aug, int64_t rows, int64_t stride_words)
{
	return guarded([&]() -> int {
	MatrixInput in; in.h_words = reinterpret_cast<const u64 *>(aug); in.stride = stride_words;
	int rc = check_append_args(h, in, rows);
	if (!rc) rc = check_device(h->device);
	if (rc) return rc;
	return factor_append(h, in, rows, nullptr);
	});
}

int gf2bv_factor_append_digits(gf2bv_factor *h, const uint32_t *digits, const int64_t *digit_off, int bits_per_digit, int64_t rows)
{
	return guarded([&]() -> int {
	if (!digit_off) return fail(GF2BV_ERR_ARG, "null pointer");
	MatrixInput in; in.h_digits = digits; in.h_off = reinterpret_cast<const i64 *>(digit_off); in.bpd = bits_per_digit;
	int rc = check_append_args(h, in, rows);
	if (!rc) rc = check_device(h->device);
	if (rc) return rc;
	return factor_append(h, in, rows, nullptr);
	});
}

int gf2bv_factor_append_device(gf2bv_factor *h, const void *d_aug, int64_t rows, int64_t stride_words, void *stream)
{
	return guarded([&]() -> int {
	MatrixInput in; in.d_words = (const u64 *)d_aug; in.stride = stride_words;
	int rc = check_append_args(h, in, rows);
	if (!rc) rc = check_device(h->device);
	if (rc) return rc;
	return factor_append(h, in, rows, (hipStream_t)stream);
	});
}

int64_t gf2bv_factor_rows(const gf2bv_factor *h)
{
	if (!h) return -1;
	std::lock_guard<std::mutex> lk(h->mu);
	return !h->failed ? h->rows : -1;
}

int gf2bv_factor_copy(gf2bv_factor *h, gf2bv_factor **out)
{
	return guarded([&]() -> int {
	if (!h || !out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	if (h->failed) return fail(GF2BV_ERR_ARG, kFailedHandle);
	return factor_copy(h, out);
	});
}

// ---- result accessors ----------------------------------------------------------------------------
int gf2bv_result_status(const gf2bv_result *r) { return r ? r->status : -1; }
int64_t gf2bv_result_rank(const gf2bv_result *r) { return r ? r->rank : -1; }
int64_t gf2bv_result_dimension(const gf2bv_result *r) { return r ? r->dim : -1; }
int64_t gf2bv_result_words(const gf2bv_result *r) { return r ? r->cw : -1; }
int gf2bv_result_origin(const gf2bv_result *r, uint64_t *o)
{
	if (!r || !o) return fail(GF2BV_ERR_ARG, "null pointer");
	memcpy(o, r->origin.data(), sizeof(u64) * r->cw);
	return GF2BV_OK;
}
int gf2bv_result_basis(const gf2bv_result *r, uint64_t *o)
{
	if (!r || (!o && !r->basis.empty())) return fail(GF2BV_ERR_ARG, "null pointer");
	if (!r->basis.empty()) memcpy(o, r->basis.data(), sizeof(u64) * r->basis.size());
	return GF2BV_OK;
}
int gf2bv_result_pivots(const gf2bv_result *r, int32_t *o)
{
	if (!r || (!o && !r->pivots.empty())) return fail(GF2BV_ERR_ARG, "null pointer");
	if (!r->pivots.empty()) memcpy(o, r->pivots.data(), sizeof(int32_t) * r->pivots.size());
	return GF2BV_OK;
}
int gf2bv_result_stats(const gf2bv_result *r, gf2bv_stats *o)
{
	if (!r || !o) return fail(GF2BV_ERR_ARG, "null pointer");
	*o = r->stats;
	return GF2BV_OK;
}
void gf2bv_result_free(gf2bv_result *r) { delete r; }

void gf2bv_space_combine(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words,
                         const uint64_t *selector, int64_t selector_words, uint64_t *o)
{
	for (i64 w = 0; w < words; w++) o[w] = origin[w];
	for (i64 i = 0; i < dimension && (i >> 6) < selector_words; i++)
		if ((selector[i >> 6] >> (i & 63)) & 1)
			for (i64 w = 0; w < words; w++) o[w] ^= basis[i * words + w];
}

// ---- column-slab solve: ONE system over several GPUs ---------------------------------
// Rank r of `world` owns the column tiles t with t % world == r (cyclic: the trailing matrix shrinks from the left).
// Per block of G panels:
//   * the rank that owns the tile of the block's window runs the panel path there (gf2bv_slab_factor) -- exactly
//     the single-GPU kernels on its compact window, the window of the NEXT block it owns being carried forward by
//     k_prio_window as before -- and exports the block's records: SolveState, alive bound, PanelRec / PanelAux of its
//     panels and the per-row multipliers (G x rows x 8 bytes): the payload of ONE broadcast over xGMI;
//   * every rank imports the payload (gf2bv_slab_apply) and runs k_block_trsm + k_update on the tiles it owns.
// After the last block each rank moves its pivot rows' parked window words into its tiles (gf2bv_slab_finish_local);
// the ranks' tiles are then gathered on one rank (the caller's collective: the working matrix is the caller's
// buffer), which has every record and finishes like a single-GPU solve (gf2bv_slab_solve: consistency check,
// back-substitution, export).  The communication is the caller's (torch.distributed: RCCL on GPUs, gloo in the CPU-side
// tests): this library stays free of it, like the rest of the C ABI.
struct gf2bv_slab {
	Solver S;
	size_t payload_bytes = 0;
	size_t o_blk = 0, o_pan = 0, o_aux = 0, o_mult = 0;
	int next_prio = 0;         // k_prio_window(b) has been enqueued for all b < next_prio (on this rank, where it owns the next window)
	// stream-ordered factor / apply (gf2bv_slab_factor_on / _apply_on): hand-overs between the caller's collective stream and
	// the library's panel stream
	// the panel stream, per payload buffer (block parity): [records exported, collective enqueued, records imported]
	hipEvent_t ev_factored[2] = { nullptr, nullptr }, ev_bcast[2] = { nullptr, nullptr }, ev_imported[2] = { nullptr, nullptr };
	bool bcast_seen[2] = { false, false }, import_seen[2] = { false, false };
	~gf2bv_slab()
	{
		if (S.sA) (void)hipStreamSynchronize(S.sA);       // (nothing that waits on these events may still be queued)
		if (S.sB) (void)hipStreamSynchronize(S.sB);
		for (int k = 0; k < 2; k++) for (hipEvent_t e : { ev_factored[k], ev_bcast[k], ev_imported[k] }) pool().release_event(e, false);
	}
};

namespace {
int slab_owner_of_block(const Solver &S, int b) { return ((b * S.impl->G) >> GF2_OWN_LOG) % S.world; }
}

int gf2bv_slab_open(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words, void *d_work, int64_t work_words,
                    int world, int rank, int device, gf2bv_slab **out)
{
	return guarded([&]() -> int {
	if (!out || !d_aug || !d_work || world < 1 || rank < 0 || rank >= world) return fail(GF2BV_ERR_ARG, "bad slab arguments");
	*out = nullptr;
	MatrixInput in; in.d_words = (const u64 *)d_aug; in.stride = stride_words;
	int rc = check_matrix_input(in, rows, cols, GF2BV_MODE_SINGLE);
	if (rc) return rc;
	if ((uintptr_t)d_work & 15) return fail(GF2BV_ERR_ARG, "the working matrix needs 16-byte alignment");
	if (work_words < gf2bv_slab_work_words(rows, cols)) return fail(GF2BV_ERR_ARG, "working matrix too small (gf2bv_slab_work_words)");
	rc = check_device(device);
	if (rc) return rc;
	gf2bv_slab *h = new gf2bv_slab();
	Solver &S = h->S;
	S.t_begin = std::chrono::steady_clock::now();
	S.device = device;
	hipError_t e = pool().stream(&S.sA, device, false);
	if (e != hipSuccess) { delete h; return fail(GF2BV_ERR_HIP, "hipStreamCreate", e); }
	S.own_sA = true;
	S.src = (const u64 *)d_aug;
	S.rows = rows; S.cols = cols; S.stride = stride_words; S.mode = GF2BV_MODE_SINGLE;
	S.world = world; S.wrank = rank;
	S.M = (u64 *)d_work; S.ext_M = true;
	rc = solver_alloc(S);                           // (converts the whole input: tiles of other ranks are simply never touched again)
	if (rc == GF2BV_OK) rc = enqueue_forward_begin(S, slab_owner_of_block(S, 0) == rank);
	if (rc != GF2BV_OK) { delete h; return rc; }
	const i64 R = std::max<i64>(1, S.rows);
	const int G = S.impl->G;
	size_t off = 0;
	auto carve = [&](size_t bytes) { size_t at = off; off += round256(bytes); return at; };
	(void)carve(sizeof(SolveState)); h->o_blk = carve(sizeof(int)); h->o_pan = carve(sizeof(PanelRec) * G);
	h->o_aux = carve(sizeof(PanelAux) * G); h->o_mult = carve(sizeof(u64) * G * mult_rows(R));
	h->payload_bytes = off;
	for (int k = 0; k < 2; k++)
		for (hipEvent_t *e : { &h->ev_factored[k], &h->ev_bcast[k], &h->ev_imported[k] })
			if (pool().event(e, false) != hipSuccess) { delete h; return fail(GF2BV_ERR_HIP, "hipEventCreate"); }
	*out = h;
	return GF2BV_OK;
	});
}

int64_t gf2bv_slab_work_words(int64_t rows, int64_t cols)
{
	const i64 wt = (cols + 1 + 63) / 64, ntiles = tiles_for(wt);
	return ntiles * TW * slab_rows(rows);
}
int64_t gf2bv_slab_tiles(int64_t cols) { return tiles_for((cols + 1 + 63) / 64) * TW >> GF2_OWN_LOG; }      // ownership units of 8 words
int64_t gf2bv_slab_blocks(const gf2bv_slab *h) { return h ? h->S.nblocks : -1; }
int gf2bv_slab_owner(const gf2bv_slab *h, int block) { return h ? slab_owner_of_block(h->S, block) : -1; }
int64_t gf2bv_slab_payload_bytes(const gf2bv_slab *h) { return h ? (int64_t)h->payload_bytes : -1; }

// records of block b <-> payload, one launch on `st` (export: to_payload)
static int slab_copy_records(gf2bv_slab *h, int b, char *P, bool to_payload, hipStream_t st)
{
	Solver &S = h->S;
	const BlockGeom g = block_geom(S, b);
	const int G = S.impl->G;
	static_assert(sizeof(SolveState) % 4 == 0 && sizeof(PanelRec) % 4 == 0 && sizeof(PanelAux) % 4 == 0, "4-byte copy units");
	struct { void *rec; size_t off, bytes; } seg[5] = {
		{ S.st, 0, sizeof(SolveState) }, { S.blk_first + b, h->o_blk, sizeof(int) }, { S.panels + g.j0, h->o_pan, sizeof(PanelRec) * g.gb },
		{ S.aux + g.j0, h->o_aux, sizeof(PanelAux) * g.gb }, { g.mset, h->o_mult, sizeof(u64) * G * mult_rows(S.rows) } };
	SlabSegs sg;
	size_t total = 0;
	for (int k = 0; k < 5; k++) {
		sg.s[k].src = to_payload ? seg[k].rec : (void *)(P + seg[k].off);
		sg.s[k].dst = to_payload ? (void *)(P + seg[k].off) : seg[k].rec;
		sg.s[k].bytes = (unsigned)seg[k].bytes;
		total += seg[k].bytes;
	}
	const unsigned wgs = (unsigned)std::min<size_t>(256, std::max<size_t>(1, total / 16 / 256 / 4));
	k_slab_copy<<<dim3(wgs), dim3(256), 0, st>>>(sg);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// Owner of block b: (carry its window forward,) factorise it, export the records into d_payload.
// Synchronous form (host_sync): returns when the payload is complete.  Stream-ordered form: `stream` is the stream the
// caller's collective runs on; the export is ONE launch on the panel stream behind the panel path, `stream` is made to wait
// for it and the call returns at once -- a broadcast enqueued on `stream` afterwards sends finished records, and the panel
// stream never waits for the collective: the caller alternates TWO payload buffers (block b uses buffer b & 1), so that the
// export of block b + 1 does not have to wait for the broadcast of block b (only for that of block b - 1, long gone).
static int slab_factor_on(gf2bv_slab *h, int b, void *d_payload, hipStream_t stream, bool host_sync)
{
	if (!h || !d_payload || b < 0 || b >= h->S.nblocks) return fail(GF2BV_ERR_ARG, "bad block");
	Solver &S = h->S;
	if (slab_owner_of_block(S, b) != S.wrank) return fail(GF2BV_ERR_ARG, "this rank does not own the block's window");
	HIPCHK(hipSetDevice(S.device));
	int rc;
	// the window of block b: carried forward from block b-1's records (imported by gf2bv_slab_apply(b-1)) -- needs this
	// rank's bulk update of block b-2, nothing newer: the look-ahead of the single-GPU solve, per owner
	if (b > 0 && (rc = enqueue_block_prio(S, b - 1))) return rc;
	if ((rc = enqueue_block_panel(S, b))) return rc;
	if (S.world == 1 && !host_sync) return GF2BV_OK;       // nobody imports: the records stay where they are
	const int par = b & 1;
	// the buffer of this parity: last read by the broadcast of block b - 2 on the caller's stream (recorded in slab_apply_on)
	if (!host_sync && h->bcast_seen[par]) HIPCHK(hipStreamWaitEvent(S.sA, h->ev_bcast[par], 0));
	if ((rc = slab_copy_records(h, b, (char *)d_payload, true, S.sA))) return rc;
	if (host_sync) HIPCHK(hipStreamSynchronize(S.sA));
	else {
		HIPCHK(hipEventRecord(h->ev_factored[par], S.sA));
		HIPCHK(hipStreamWaitEvent(stream, h->ev_factored[par], 0));
	}
	return GF2BV_OK;
}

// Every rank: take block b's records (the other ranks import them from the broadcast payload, which `stream` has produced),
// then TRSM + bulk update of the tiles this rank owns.  Asynchronous.
static int slab_apply_on(gf2bv_slab *h, int b, const void *d_payload, hipStream_t stream, bool host_sync)
{
	if (!h || !d_payload || b < 0 || b >= h->S.nblocks) return fail(GF2BV_ERR_ARG, "bad block");
	Solver &S = h->S;
	HIPCHK(hipSetDevice(S.device));
	const BlockGeom g = block_geom(S, b);
	const int par = b & 1;
	if (!host_sync && S.world > 1) {               // "the collective of block b has read / written buffer b & 1"
		HIPCHK(hipEventRecord(h->ev_bcast[par], stream));
		h->bcast_seen[par] = true;
	}
	if (slab_owner_of_block(S, b) != S.wrank) {
		if (!host_sync) HIPCHK(hipStreamWaitEvent(S.sA, h->ev_bcast[par], 0));      // the payload is what `stream` holds now
		// the multiplier set of block b was last read by this rank's bulk update of block b - nsets
		if (b >= S.nsets) HIPCHK(hipStreamWaitEvent(S.sA, S.waitPrio[b - S.nsets], 0));
		int rc = slab_copy_records(h, b, (char *)const_cast<void *>(d_payload), false, S.sA);
		if (rc) return rc;
		k_import_marks<<<dim3(1), dim3(256), 0, S.sA>>>(g.j0, g.gb, S.panels, S.aux, S.died, S.pivcol, S.urow);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(S.evA[b], S.sA));
		// the payload buffer may be overwritten once the import has read it: after this returns (host_sync), or by what the
		// caller enqueues on `stream` behind the wait below -- placed one call LATER (the import of the previous block: the
		// buffer it read is the one the next-but-one collective writes), so that the collective stream stays a block ahead
		if (host_sync) HIPCHK(hipStreamSynchronize(S.sA));
		else { HIPCHK(hipEventRecord(h->ev_imported[par], S.sA)); h->import_seen[par] = true; }
	}
	if (!host_sync && h->import_seen[par ^ 1]) HIPCHK(hipStreamWaitEvent(stream, h->ev_imported[par ^ 1], 0));
	return enqueue_block_bulk(S, b);
}

int gf2bv_slab_factor(gf2bv_slab *h, int b, void *d_payload)
{
	return guarded([&]() -> int { return slab_factor_on(h, b, d_payload, nullptr, true); });
}
int gf2bv_slab_apply(gf2bv_slab *h, int b, const void *d_payload)
{
	return guarded([&]() -> int { return slab_apply_on(h, b, d_payload, nullptr, true); });
}
int gf2bv_slab_factor_on(gf2bv_slab *h, int b, void *d_payload, void *stream)
{
	return guarded([&]() -> int { return slab_factor_on(h, b, d_payload, (hipStream_t)stream, false); });
}
int gf2bv_slab_apply_on(gf2bv_slab *h, int b, const void *d_payload, void *stream)
{
	return guarded([&]() -> int { return slab_apply_on(h, b, d_payload, (hipStream_t)stream, false); });
}

// After the last block: this rank's tiles are final (pivot rows' parked window words moved in); synchronous.
int gf2bv_slab_finish_local(gf2bv_slab *h)
{
	return guarded([&]() -> int {
	if (!h) return fail(GF2BV_ERR_ARG, "null pointer");
	Solver &S = h->S;
	HIPCHK(hipSetDevice(S.device));
	int rc = enqueue_forward_join(S);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(S.sA));
	HIPCHK(hipStreamSynchronize(S.sB));
	return GF2BV_OK;
	});
}

// On the rank that holds ALL tiles (after the caller's gather): consistency check, back-substitution, export -- the tail
// of a single-GPU solve_one.
int gf2bv_slab_solve(gf2bv_slab *h, gf2bv_result **out)
{
	return guarded([&]() -> int {
	if (!h || !out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	Solver &S = h->S;
	S.kn.refresh();
	HIPCHK(hipSetDevice(S.device));
	int rc = enqueue_check_rhs(S);
	if (rc == GF2BV_OK) rc = enqueue_backward_parity(S, { (int)S.cols });
	if (rc) return rc;
	rc = solver_finish(S, out);
	// (the elimination state of a slab handle cannot be replayed from here: an expired gate is an error, not a retry)
	if (rc == GF2BV_RETRY_EVENTS) return fail(GF2BV_ERR_HIP, "a stream hand-over gate timed out on the device");
	return rc;
	});
}

void gf2bv_slab_close(gf2bv_slab *h)
{
	if (!h) return;
	(void)hipSetDevice(h->S.device);
	delete h;
}

// ---- AffineSpace on the device: bulk enumeration ------------------------------------------------
struct gf2bv_space {
	int device = 0;
	int64_t dim = 0, words = 0;
	u64 *d_origin = nullptr, *d_basis = nullptr;
	u64 *d_out = nullptr;
	u64 *h_out = nullptr;         // pinned staging: the device-to-host copy runs at link speed, and callers that pass no
	size_t out_words = 0;         // output pointer read the elements straight from it (gf2bv_space_buffer)
	hipStream_t st = nullptr;
};

int gf2bv_space_open(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int device,
                     gf2bv_space **out)
{
	return guarded([&]() -> int {
	if (!out || !origin || dimension < 0 || words <= 0 || (dimension > 0 && !basis)) return fail(GF2BV_ERR_ARG, "bad space");
	*out = nullptr;
	int rc = check_device(device);
	if (rc) return rc;
	gf2bv_space *sp = new gf2bv_space();
	sp->device = device; sp->dim = dimension; sp->words = words;
	auto bail = [&](hipError_t e, const char *what) { gf2bv_space_close(sp); return fail(GF2BV_ERR_HIP, what, e); };
	hipError_t e = pool().stream(&sp->st, device, false);
	if (e != hipSuccess) return bail(e, "hipStreamCreate");
	if ((e = pool().alloc((void **)&sp->d_origin, sizeof(u64) * words, device)) != hipSuccess) return bail(e, "hipMalloc");
	if ((e = pool().alloc((void **)&sp->d_basis, sizeof(u64) * std::max<i64>(1, dimension * words), device)) != hipSuccess) return bail(e, "hipMalloc");
	if ((e = hipMemcpyAsync(sp->d_origin, origin, sizeof(u64) * words, hipMemcpyHostToDevice, sp->st)) != hipSuccess) return bail(e, "hipMemcpy");
	if (dimension > 0 && (e = hipMemcpyAsync(sp->d_basis, basis, sizeof(u64) * dimension * words, hipMemcpyHostToDevice, sp->st)) != hipSuccess)
		return bail(e, "hipMemcpy");
	if ((e = hipStreamSynchronize(sp->st)) != hipSuccess) return bail(e, "hipStreamSynchronize");      // the caller's buffers may go away
	*out = sp;
	return GF2BV_OK;
	});
}

int gf2bv_space_enumerate(gf2bv_space *sp, uint64_t first, int64_t count, int gray, uint64_t *out_words)
{
	return guarded([&]() -> int {
	if (!sp || count < 0) return fail(GF2BV_ERR_ARG, "null pointer");
	if (count == 0) return GF2BV_OK;
	HIPCHK(hipSetDevice(sp->device));
	const size_t need = (size_t)count * sp->words;
	if (need > sp->out_words) {
		pool().release(sp->d_out); sp->d_out = nullptr; sp->out_words = 0;
		if (sp->h_out) { (void)hipHostFree(sp->h_out); sp->h_out = nullptr; }
		HIPCHK(pool().alloc((void **)&sp->d_out, sizeof(u64) * need, sp->device));
		HIPCHK(hipHostMalloc((void **)&sp->h_out, sizeof(u64) * need, hipHostMallocDefault));
		sp->out_words = need;
	}
	const dim3 grid((unsigned)((sp->words + 255) / 256), (unsigned)std::min<i64>(count, 65535));
	k_space_enumerate<<<grid, dim3(256), 0, sp->st>>>(sp->d_origin, sp->d_basis, (int)std::min<i64>(sp->dim, 64), sp->words,
	                                                  (u64)first, (i64)count, gray, sp->d_out);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(sp->h_out, sp->d_out, sizeof(u64) * need, hipMemcpyDeviceToHost, sp->st));
	HIPCHK(hipStreamSynchronize(sp->st));
	if (out_words) memcpy(out_words, sp->h_out, sizeof(u64) * need);
	return GF2BV_OK;
	});
}

const uint64_t *gf2bv_space_buffer(const gf2bv_space *sp) { return sp ? reinterpret_cast<const uint64_t *>(sp->h_out) : nullptr; }

void gf2bv_space_close(gf2bv_space *sp)
{
	if (!sp) return;
	(void)hipSetDevice(sp->device);
	if (sp->st) (void)hipStreamSynchronize(sp->st);
	pool().release(sp->d_origin); pool().release(sp->d_basis); pool().release(sp->d_out);
	if (sp->h_out) (void)hipHostFree(sp->h_out);
	if (sp->st) pool().release_stream(sp->st, sp->device, false);
	delete sp;
}

// ---- synthetic + residual + buffers --------------------------------------------------------------
int gf2bv_synth_device(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words, uint64_t seed,
                       int device, void *stream)
{
	if (!d_aug || rows < 0 || cols <= 0 || stride_words < (cols + 1 + 63) / 64 || rows >= (1ll << 20) - 1)
		return fail(GF2BV_ERR_ARG, "bad synthetic shape");
	int rc = check_device(device);
	if (rc) return rc;
	if (rows == 0) return GF2BV_OK;
	hipLaunchKernelGGL(k_synth, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
	                   (u64 *)d_aug, (i64)rows, (i64)cols, (i64)stride_words, (u64)seed);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

int gf2bv_residual_device(const void *d_aug, int64_t rows, int64_t cols, int64_t stride_words,
                          const uint64_t *x_words, int device, void *stream, int64_t *bad_rows)
{
	if (!d_aug || !x_words || !bad_rows || cols <= 0) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_device(device);
	if (rc) return rc;
	const i64 cw = (cols + 63) / 64;
	u64 *dx = nullptr, *dbad = nullptr;
	HIPCHK(hipMalloc(&dx, sizeof(u64) * cw));
	HIPCHK(hipMalloc(&dbad, sizeof(u64)));
	hipStream_t s = (hipStream_t)stream;
	HIPCHK(hipMemcpyAsync(dx, x_words, sizeof(u64) * cw, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemsetAsync(dbad, 0, sizeof(u64), s));
	if (rows > 0)
		hipLaunchKernelGGL(k_residual, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s,
		                   (const u64 *)d_aug, (i64)rows, (i64)cols, (i64)stride_words, dx, dbad);
	u64 h = 0;
	HIPCHK(hipMemcpyAsync(&h, dbad, sizeof h, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	(void)hipFree(dx); (void)hipFree(dbad);
	*bad_rows = (int64_t)h;
	return GF2BV_OK;
}

// Registers (VGPRs per lane) and static LDS of the kernels that must fit on a CU TOGETHER: the default bulk-update instance
// and the panel-path kernels that run beside it.  out[2 k], out[2 k + 1] = registers, LDS bytes of kernel k (see
// gf2bv_hip.h for the order).
int gf2bv_kernel_resources(int device, int32_t *out, int n)
{
	return guarded([&]() -> int {
	if (!out || n < 10) return fail(GF2BV_ERR_ARG, "need room for 5 kernels");
	for (int k = 0; k < n; k++) out[k] = 0;
	int rc = check_device(device);
	if (rc) return rc;
	HIPCHK(hipSetDevice(device));
	const void *fn[5] = { (const void *)k_update16<512, false, 3, true, 512>, (const void *)k_block_fast, (const void *)k_narrow_all,
	                      (const void *)k_prio_window, (const void *)k_panel_step };
	for (int k = 0; k < 5; k++) {
		hipFuncAttributes a{};
		HIPCHK(hipFuncGetAttributes(&a, fn[k]));
		out[2 * k] = a.numRegs;
		out[2 * k + 1] = (int32_t)a.sharedSizeBytes;
	}
	if (n >= 13) {                 // the outer pass of the two-level elimination: registers, LDS, scratch bytes per lane (must be 0)
		hipFuncAttributes a{};
		HIPCHK(hipFuncGetAttributes(&a, (const void *)k_update16k_wide));       // (the default shape: 16 wavefronts under a budget of 120 registers)
		out[10] = a.numRegs; out[11] = (int32_t)a.sharedSizeBytes; out[12] = (int32_t)a.localSizeBytes;
	}
	if (n >= 15) {                 // search + narrow step in one launch (runs beside the bulk update like the two it replaces)
		hipFuncAttributes a{};
		HIPCHK(hipFuncGetAttributes(&a, (const void *)k_block_fast_narrow));
		out[13] = a.numRegs; out[14] = (int32_t)a.sharedSizeBytes;
	}
	if (n >= 17) {                 // round 5: the sparse block search (first pool size: beside the bulk update)
		hipFuncAttributes a{};
		HIPCHK(hipFuncGetAttributes(&a, (const void *)k_block_sparse<256, 4>));
		out[15] = a.numRegs; out[16] = (int32_t)a.sharedSizeBytes;
	}
	return GF2BV_OK;
	});
}

int gf2bv_stream_ceiling_device(int device, int64_t bytes, double *rmw_gbs, double *read_gbs)
{
	if (!rmw_gbs || !read_gbs || bytes < (1 << 20)) return fail(GF2BV_ERR_ARG, "bad ceiling request");
	int rc = check_device(device);
	if (rc) return rc;
	const int wgs = 2048;
	const i64 per = bytes / 16 / wgs;
	uint4 *buf = nullptr;
	unsigned *sink = nullptr;
	hipError_t e = hipMalloc(&buf, (size_t)per * wgs * 16);
	if (e != hipSuccess) return fail(GF2BV_ERR_NOMEM, "hipMalloc", e);
	HIPCHK(hipMalloc(&sink, 64));
	HIPCHK(hipMemset(buf, 1, (size_t)per * wgs * 16));
	hipEvent_t e0, e1;
	HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
	const int reps = 5;
	float ms = 0;
	k_rmw_stream<<<dim3(wgs), dim3(1024)>>>(buf, per, 5u);
	HIPCHK(hipEventRecord(e0, nullptr));
	for (int r = 0; r < reps; r++) k_rmw_stream<<<dim3(wgs), dim3(1024)>>>(buf, per, 5u);
	HIPCHK(hipEventRecord(e1, nullptr));
	HIPCHK(hipEventSynchronize(e1));
	HIPCHK(hipEventElapsedTime(&ms, e0, e1));
	*rmw_gbs = 2.0 * (double)per * wgs * 16 * reps / (ms * 1e-3) / 1e9;
	k_read_stream<<<dim3(wgs), dim3(1024)>>>(buf, per, sink);
	HIPCHK(hipEventRecord(e0, nullptr));
	for (int r = 0; r < reps; r++) k_read_stream<<<dim3(wgs), dim3(1024)>>>(buf, per, sink);
	HIPCHK(hipEventRecord(e1, nullptr));
	HIPCHK(hipEventSynchronize(e1));
	HIPCHK(hipEventElapsedTime(&ms, e0, e1));
	*read_gbs = (double)per * wgs * 16 * reps / (ms * 1e-3) / 1e9;
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	(void)hipFree(buf); (void)hipFree(sink);
	return GF2BV_OK;
}

int gf2bv_lds_clock_device(int device, double *shader_mhz, double *lds_bytes_per_clk_cu)
{
	if (!shader_mhz || !lds_bytes_per_clk_cu) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_device(device);
	if (rc) return rc;
	unsigned long long *d = nullptr, h[3] = { 0, 0, 0 };
	unsigned *sink = nullptr;
	Held H(device, nullptr);                    // (the kernels run on the null stream)
	HIPCHK(H.get((void **)&d, sizeof h));
	HIPCHK(H.get((void **)&sink, 64));
	int cus = 256;
	(void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
	k_lds_clock<<<dim3(cus), dim3(512)>>>(d, 2000, sink);                   // warm-up (clocks ramp)
	k_lds_clock<<<dim3(cus), dim3(512)>>>(d, 40000, sink);                  // ~5 ms of ds_read_b128 on every CU
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
	if (!h[1]) return fail(GF2BV_ERR_HIP, "the clock probe measured nothing");
	*shader_mhz = (double)h[0] / ((double)h[1] / 100.0);                    // real-time counter: 100 MHz
	*lds_bytes_per_clk_cu = (double)h[2] * 1024.0 / (double)h[0];           // a ds_read_b128 wave-instruction moves 1 KiB
	return GF2BV_OK;
}

int gf2bv_device_alloc(int device, int64_t bytes, void **d_ptr)
{
	if (!d_ptr || bytes < 0) return fail(GF2BV_ERR_ARG, "bad alloc request");
	int rc = check_device(device);
	if (rc) return rc;
	// (not pooled: the buffer is the caller's; but a request the device cannot serve while the pool sits on idle buffers
	// gets them first)
	hipError_t e = pool().malloc_retry(d_ptr, (size_t)std::max<i64>(bytes, 16), device);
	if (e != hipSuccess) return fail(GF2BV_ERR_NOMEM, "hipMalloc", e);
	return GF2BV_OK;
}
// ---- pinned host staging for bindings (round 5) ------------------------------------------------------------------------------
// A binding that has to assemble its input on the host (the CPython shim copies every equation's ob_digit array into one buffer)
// gets that buffer here: page-locked, so the host-to-device copy of gf2bv_solve_digits is ONE DMA instead of the runtime's
// chunk-by-chunk staging of pageable memory, and recycled between calls (no page faults on a fresh 50 MB allocation every call).
// Up to four idle buffers are kept, GF2BV_HOST_POOL_MB MiB in all at most (default 4608: the two 2 GiB chunk buffers a batched
// list-of-int call alternates between -- page-locking 800 MB anew on every call was 200 of the 270 ms of a 16-system MT19937
// batch, profiles/r05_mt_many.txt); larger ones are freed on return, gf2bv_host_pool_trim frees the idle ones.
namespace {
struct HostPool {
	std::mutex mu;
	struct Buf { void *p; size_t bytes; };
	std::vector<Buf> idle;
	std::unordered_map<void *, size_t> live;
};
HostPool *host_pool_ptr() { static HostPool *p = new HostPool(); return p; }
}
int gf2bv_host_alloc(int64_t bytes, void **h_ptr)
{
	if (!h_ptr || bytes < 0) return fail(GF2BV_ERR_ARG, "bad alloc request");
	*h_ptr = nullptr;
	const size_t need = std::max<size_t>((size_t)bytes, 64);
	HostPool &P = *host_pool_ptr();
	{
		std::lock_guard<std::mutex> lk(P.mu);
		for (size_t i = 0; i < P.idle.size(); i++)
			if (P.idle[i].bytes >= need && P.idle[i].bytes <= 2 * need + ((size_t)1 << 20)) {
				*h_ptr = P.idle[i].p; P.live[*h_ptr] = P.idle[i].bytes;
				P.idle.erase(P.idle.begin() + i);
				return GF2BV_OK;
			}
	}
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(GF2BV_ERR_NODEVICE, "no HIP device visible");
	void *p = nullptr;
	const size_t cap = need + need / 8;
	hipError_t e = hipHostMalloc(&p, cap, hipHostMallocDefault);
	if (e != hipSuccess) { (void)hipGetLastError(); return fail(GF2BV_ERR_NOMEM, "hipHostMalloc", e); }
	std::lock_guard<std::mutex> lk(P.mu);
	P.live[p] = cap;
	*h_ptr = p;
	return GF2BV_OK;
}
void gf2bv_host_free(void *h_ptr)
{
	if (!h_ptr) return;
	HostPool &P = *host_pool_ptr();
	void *drop = nullptr;
	{
		std::lock_guard<std::mutex> lk(P.mu);
		auto it = P.live.find(h_ptr);
		if (it == P.live.end()) return;
		const size_t bytes = it->second;
		P.live.erase(it);
		size_t kept = 0;
		for (const auto &b : P.idle) kept += b.bytes;
		const size_t cap_mb = (size_t)Knobs::read(Knobs::kHostPool).host_pool_mb;
		if (P.idle.size() < 4 && kept + bytes <= (cap_mb << 20)) P.idle.push_back({ h_ptr, bytes });
		else drop = h_ptr;
	}
	if (drop) (void)hipHostFree(drop);
}

int64_t gf2bv_host_pool_trim(void)
{
	HostPool &P = *host_pool_ptr();
	std::vector<HostPool::Buf> drop;
	{
		std::lock_guard<std::mutex> lk(P.mu);
		drop.swap(P.idle);
	}
	int64_t bytes = 0;
	for (const auto &b : drop) { bytes += (int64_t)b.bytes; (void)hipHostFree(b.p); }
	return bytes;
}

// The gang size gf2bv_solve_batch_* would choose for nsys systems of rows x cols with free_bytes of device memory free -- a pure
// function (no device is touched): bench.py --dry-run-ranks prints every rank's plan of the multi-GPU batch job with it.
int64_t gf2bv_plan_gang(int64_t nsys, int64_t rows, int64_t cols, int64_t free_bytes)
{
	if (nsys <= 0 || rows <= 0 || cols <= 0 || free_bytes < 0) return 0;
	return pick_gang(Knobs::read(), nsys, rows, cols, free_bytes);
}

// The environment switches as a per-call entry would parse them now, one NAME=value line each (see Knobs); no device is touched.
int gf2bv_knob_dump(char *buf, int64_t n)
{
	return catching([&]() -> int {
	const std::string s = Knobs::read().dump();
	if (!buf || (int64_t)s.size() >= n) return fail(GF2BV_ERR_ARG, "null pointer, or a buffer too small for the knob dump");
	memcpy(buf, s.c_str(), s.size() + 1);
	return GF2BV_OK;
	});
}

int64_t gf2bv_pool_trim(int device)
{
	if (check_device(device)) return -1;
	return (int64_t)pool().trim(device);
}
int64_t gf2bv_pool_idle_bytes(int device)
{
	if (device < 0) return -1;
	Pool &P = pool();
	std::lock_guard<std::mutex> lk(P.mu);
	size_t bytes = 0;
	auto bf = P.big_free.find(device);
	if (bf != P.big_free.end()) for (const Pool::Big &b : bf->second) bytes += b.bytes;
	for (auto &kv : P.free_bufs) if (kv.first.first == device) bytes += kv.first.second * kv.second.size();
	return (int64_t)bytes;
}
int gf2bv_pool_in_use(int device, int64_t out[3])
{
	if (device < 0 || !out) return -1;
	Pool &P = pool();
	std::lock_guard<std::mutex> lk(P.mu);
	out[0] = 0; out[1] = P.streams_out[device]; out[2] = P.events_out[device];
	for (const auto *m : { &P.live, &P.big_live }) for (const auto &kv : *m) out[0] += kv.second.first == device;
	return 0;
}
int gf2bv_device_free(int device, void *d_ptr)
{
	int rc = check_device(device);
	if (rc) return rc;
	HIPCHK(hipFree(d_ptr));
	return GF2BV_OK;
}
int gf2bv_device_upload(int device, void *d_dst, const void *h_src, int64_t bytes)
{
	int rc = check_device(device);
	if (rc) return rc;
	HIPCHK(hipMemcpy(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice));
	return GF2BV_OK;
}
int gf2bv_device_download(int device, void *h_dst, const void *d_src, int64_t bytes)
{
	int rc = check_device(device);
	if (rc) return rc;
	HIPCHK(hipMemcpy(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
	return GF2BV_OK;
}

#ifdef GF2_SPARSE_DEBUG
extern "C" int gf2bv_sparse_probe_read(unsigned long long *w, int reset)
{
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpyFromSymbol(w, HIP_SYMBOL(gf2_sparse_probe), sizeof(gf2_sparse_probe)));
	if (reset) { unsigned long long z[8] = { 0 }; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gf2_sparse_probe), z, sizeof z)); }
	return GF2BV_OK;
}
#endif
#ifdef GF2_STEP_PROBE
// Probe build only (tools/probe_step.py): choose the block whose panel steps are recorded, fetch the records.
int gf2bv_probe_set(int j0)
{
	HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gf2_probe_j0), &j0, sizeof(int)));
	void *p = nullptr;
	HIPCHK(hipGetSymbolAddress(&p, HIP_SYMBOL(gf2_probe_upd))); HIPCHK(hipMemset(p, 0, sizeof(gf2_probe_upd)));
	HIPCHK(hipGetSymbolAddress(&p, HIP_SYMBOL(gf2_probe_wg))); HIPCHK(hipMemset(p, 0, sizeof(gf2_probe_wg)));
	HIPCHK(hipGetSymbolAddress(&p, HIP_SYMBOL(gf2_probe_un))); HIPCHK(hipMemset(p, 0, sizeof(gf2_probe_un)));
	return GF2BV_OK;
}
int gf2bv_probe_read_update(unsigned long long *upd)
{
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpyFromSymbol(upd, HIP_SYMBOL(gf2_probe_upd), sizeof(gf2_probe_upd)));
	return GF2BV_OK;
}
int gf2bv_probe_read_gj(unsigned long long *w)
{
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpyFromSymbol(w, HIP_SYMBOL(gf2_probe_gj), sizeof(gf2_probe_gj)));
	return GF2BV_OK;
}
int gf2bv_probe_read_fast(unsigned long long *w)
{
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpyFromSymbol(w, HIP_SYMBOL(gf2_probe_fast), sizeof(gf2_probe_fast)));
	return GF2BV_OK;
}
int gf2bv_probe_read_wave(unsigned long long *w)
{
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpyFromSymbol(w, HIP_SYMBOL(gf2_probe_wave), sizeof(gf2_probe_wave)));
	return GF2BV_OK;
}
int gf2bv_probe_read(unsigned long long *wg, unsigned long long *un)
{
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpyFromSymbol(wg, HIP_SYMBOL(gf2_probe_wg), sizeof(gf2_probe_wg)));
	HIPCHK(hipMemcpyFromSymbol(un, HIP_SYMBOL(gf2_probe_un), sizeof(gf2_probe_un)));
	return GF2BV_OK;
}
#endif

}  // extern "C"

// ---- quadratic search: the consistent points of a linearised quadratic system's solution space --------------------------
//   A space x(c) = o ^ B c over n linear coordinates followed by the n(n-1)/2 product coordinates
// (pair (i, j), j < i, at n + i(i-1)/2 + j).  Step 1: column operations T split B into A (r vectors, independent linear
// parts) and K (d - r vectors, zero linear parts, RREF over the product coordinates, pivots P).  Step 2: a choice c_a of the
// A coefficients extends to a consistent point iff, at every product coordinate t outside P, v_t = XOR_{p in P} v_p K_p[t]
// where v_s = l_i l_j ^ q_s -- one quadratic form in r variables per such t (k_quad_forms); affine forms are eliminated on
// the host, one variable each.  Step 3: r_eff <= max_enum: k_quad_search + k_forms_check<2>; above: relinearise (the forms are
// the equations of a QuadraticSystem of r_eff unknowns, solved by this library) and repeat on that space while r_eff falls.
namespace {

constexpr i64 kQuadMaxRank = 256;            // larger projection ranks are not reduced (the forms would hold (r + 1)^2 bits each)
constexpr i64 kQuadMaxPoints = 1ll << 22;    // consistent points collected (and ordered) at most
constexpr i64 kQuadMaxCand = 1ll << 22;      // candidates of the first search pass kept for the second (more: one fused pass)
constexpr int kQuadMaxEnum = 40;
constexpr int kQuadMaxDepth = 8;

inline bool qbit(const u64 *v, i64 i) { return (v[i >> 6] >> (i & 63)) & 1; }
inline void qflip(u64 *v, i64 i) { v[i >> 6] ^= 1ull << (i & 63); }
inline void qxor(u64 *d, const u64 *s, i64 n) { for (i64 k = 0; k < n; k++) d[k] ^= s[k]; }
inline bool qzero(const u64 *v, i64 n) { for (i64 k = 0; k < n; k++) if (v[k]) return false; return true; }
// d ^= s restricted to the bits above `e` (words of W)
inline void qxor_above(u64 *d, const u64 *s, i64 e, i64 W)
{
	const i64 w0 = (e + 1) >> 6;
	if (w0 >= W) return;
	d[w0] ^= s[w0] & (~0ull << ((e + 1) & 63));
	for (i64 w = w0 + 1; w < W; w++) d[w] ^= s[w];
}

struct QuadTimes { double reduce = 0, forms = 0, affine = 0, search = 0, relin = 0, total = 0; i64 levels = 0, candidates = 0; };
thread_local QuadTimes g_quad_times;

inline double ms_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct QuadPlan {
	i64 n = 0, S = 0, N = 0, words = 0, d = 0, dw = 1, r = 0, W = 1;
	std::vector<u64> origin, V, T;       // V: d x words (A rows 0..r-1, then K rows); T: d x dw (row j = original coefficients of V_j)
	std::vector<i64> kpiv;               // product coordinate (0..S-1) of the pivot of K row k
	i64 m0 = 0;                          // forms before the affine elimination: one per product coordinate outside P
	std::vector<u64> lin, qaff;          // n x W, S x W (inputs of k_quad_forms, with the pair decode and the supports)
	std::vector<int> pair_i, pair_j, sup_idx;
	std::vector<i64> sup_off;
	std::vector<u64> M;                  // m0 x (r + 1) x W canonical forms over matrix variables 1..r
	bool inconsistent = false;
	std::vector<int> sub_var;            // affine elimination: variable, and its value as an affine form (W words, bit 0 = 1)
	std::vector<u64> sub_sigma;
	std::vector<int> alive;              // matrix variable of effective variable v
	i64 reff = 0, fw = 1, m = 0;
	std::vector<u64> forms;              // m x fw, equation-int layout over reff unknowns
};

// step 1 and the inputs of step 2
// (S product coordinates behind the n linear ones: C(n,2) here, C(n,2) + C(n,3) for the cubic search)
void quad_reduce(QuadPlan &P, const u64 *origin, const u64 *basis, i64 d, i64 words, i64 n, i64 S)
{
	P.n = n; P.S = S; P.N = n + P.S; P.words = words; P.d = d; P.dw = std::max<i64>(1, (d + 63) / 64);
	P.origin.assign(origin, origin + words);
	P.V.assign(basis, basis + d * words);
	P.T.assign((size_t)(d * P.dw), 0);
	for (i64 j = 0; j < d; j++) qflip(&P.T[j * P.dw], j);
	auto row = [&](i64 i) { return &P.V[i * words]; };
	auto swap_rows = [&](i64 a, i64 b) {
		std::swap_ranges(row(a), row(a) + words, row(b));
		std::swap_ranges(&P.T[a * P.dw], &P.T[a * P.dw] + P.dw, &P.T[b * P.dw]);
	};
	auto pivot_on = [&](i64 c, i64 at, i64 lo) -> bool {       // pivot of column c at row `at` (rows >= lo searched / cleared)
		i64 p = -1;
		for (i64 i = at; i < d; i++) if (qbit(row(i), c)) { p = i; break; }
		if (p < 0) return false;
		if (p != at) swap_rows(p, at);
		const i64 w0 = c >> 6;              // (the pivot row is zero left of c)
		for (i64 i = lo; i < d; i++)
			if (i != at && qbit(row(i), c)) { qxor(row(i) + w0, row(at) + w0, words - w0); qxor(&P.T[i * P.dw], &P.T[at * P.dw], P.dw); }
		return true;
	};
	i64 rk = 0;
	for (i64 c = 0; c < n && rk < d; c++) if (pivot_on(c, rk, 0)) rk++;
	P.r = rk;
	for (i64 c = n; c < P.N && rk < d; c++) if (pivot_on(c, rk, P.r)) { P.kpiv.push_back(c - n); rk++; }
}

void quad_inputs(QuadPlan &P)
{
	const i64 n = P.n, S = P.S, r = P.r, words = P.words;
	P.W = (r + 64) / 64;
	const i64 W = P.W;
	P.lin.assign((size_t)(std::max<i64>(n, 1) * W), 0);
	P.qaff.assign((size_t)(std::max<i64>(S, 1) * W), 0);
	for (i64 i = 0; i < P.N; i++) {
		u64 *f = i < n ? &P.lin[i * W] : &P.qaff[(i - n) * W];
		if (qbit(P.origin.data(), i)) f[0] |= 1;
		for (i64 a = 0; a < r; a++) if (qbit(&P.V[a * words], i)) qflip(f, a + 1);
	}
	P.pair_i.resize((size_t)std::max<i64>(S, 1)); P.pair_j.resize((size_t)std::max<i64>(S, 1));
	for (i64 i = 1, s = 0; i < n; i++) for (i64 j = 0; j < i; j++, s++) { P.pair_i[s] = (int)i; P.pair_j[s] = (int)j; }
	// forms: one per product coordinate t outside P, numbered in coordinate order; support of form t = {t} and the pivots p
	// of the K rows that have a bit at t (a list per form: sup_idx[sup_off[t] .. sup_off[t + 1]))
	std::vector<i64> form_of((size_t)std::max<i64>(S, 1), 0);
	for (i64 p : P.kpiv) form_of[p] = -1;
	P.m0 = 0;
	for (i64 s = 0; s < S; s++) if (form_of[s] == 0) form_of[s] = P.m0++;
	std::vector<std::pair<i64, int>> hits;          // (form, pivot coordinate) for every K bit outside P
	for (size_t k = 0; k < P.kpiv.size(); k++) {
		const u64 *kv = &P.V[(r + (i64)k) * words];
		for (i64 w = n >> 6; w < words; w++) {
			for (u64 bits = kv[w]; bits; bits &= bits - 1) {
				const i64 c = w * 64 + __builtin_ctzll(bits);
				if (c < n || c >= P.N) continue;
				const i64 t = form_of[c - n];
				if (t >= 0) hits.push_back({t, (int)P.kpiv[k]});
			}
		}
	}
	P.sup_off.assign((size_t)(P.m0 + 1), 0);
	for (i64 t = 0; t < P.m0; t++) P.sup_off[t + 1] = 1;
	for (auto &h : hits) P.sup_off[h.first + 1]++;
	for (i64 t = 0; t < P.m0; t++) P.sup_off[t + 1] += P.sup_off[t];
	P.sup_idx.assign((size_t)std::max<i64>(1, P.sup_off[P.m0]), 0);
	std::vector<i64> at(P.sup_off.begin(), P.sup_off.end() - 1);
	for (i64 s = 0; s < S; s++) if (form_of[s] >= 0) P.sup_idx[at[form_of[s]]++] = (int)s;
	for (auto &h : hits) P.sup_idx[at[h.first]++] = h.second;
}

// the host twin of k_quad_forms (gf2bv_quad_plan never touches a device)
void quad_forms_host(QuadPlan &P)
{
	const i64 r = P.r, W = P.W, cells = (r + 1) * W;
	P.M.assign((size_t)(std::max<i64>(P.m0, 1) * cells), 0);
	std::vector<u64> acc((size_t)cells);
	for (i64 t = 0; t < P.m0; t++) {
		std::fill(acc.begin(), acc.end(), 0);
		for (i64 k = P.sup_off[t]; k < P.sup_off[t + 1]; k++) {
			const i64 s = P.sup_idx[k];
			const u64 *li = &P.lin[(i64)P.pair_i[s] * W], *lj = &P.lin[(i64)P.pair_j[s] * W];
			for (i64 a = 0; a <= r; a++) if (qbit(li, a)) qxor(&acc[a * W], lj, W);
			qxor(&acc[0], &P.qaff[s * W], W);
		}
		u64 *o = &P.M[t * cells];
		for (i64 a = 0; a <= r; a++)
			for (i64 b = a; b <= r; b++) {
				if (a == 0) {
					const bool v = b == 0 ? qbit(&acc[0], 0) : (qbit(&acc[0], b) ^ qbit(&acc[b * W], 0) ^ qbit(&acc[b * W], b));
					if (v) qflip(&o[0], b);
				} else if (b > a && (qbit(&acc[a * W], b) ^ qbit(&acc[b * W], a))) {
					qflip(&o[a * W], b);
				}
			}
	}
}

// the affine elimination of step 2 and the final forms (equation-int layout over the r_eff variables left)
void quad_affine(QuadPlan &P)
{
	const i64 r = P.r, W = P.W, cells = (r + 1) * W;
	std::vector<char> live((size_t)std::max<i64>(P.m0, 1), 1), quad((size_t)std::max<i64>(P.m0, 1), 0);
	auto F = [&](i64 f) { return &P.M[f * cells]; };
	auto classify = [&](i64 f) -> bool {           // false: the constant 1 (no point at all)
		quad[f] = !qzero(F(f) + W, r * W);
		if (quad[f]) return true;
		const u64 *r0 = F(f);
		bool lin = (r0[0] & ~1ull) != 0;
		for (i64 w = 1; w < W && !lin; w++) lin = r0[w] != 0;
		if (!lin) { live[f] = 0; return (r0[0] & 1) == 0; }
		return true;
	};
	for (i64 f = 0; f < P.m0; f++) if (!classify(f)) { P.inconsistent = true; break; }
	std::vector<char> var_alive((size_t)(r + 1), 1);
	std::vector<u64> u((size_t)W), sig((size_t)W), su((size_t)W);
	for (i64 f = 0; !P.inconsistent && f < P.m0; f++) {
		if (!live[f] || quad[f]) continue;
		u64 *r0 = F(f);
		i64 a = -1;
		for (i64 w = W - 1; w >= 0 && a < 0; w--) if (r0[w] & (w ? ~0ull : ~1ull)) a = w * 64 + 63 - __builtin_clzll(r0[w] & (w ? ~0ull : ~1ull));
		std::copy(r0, r0 + W, sig.begin());
		qflip(sig.data(), a);                      // c_a = sigma(c): constant bit 0, variables above
		live[f] = 0;
		var_alive[a] = 0;
		P.sub_var.push_back((int)a);
		P.sub_sigma.insert(P.sub_sigma.end(), sig.begin(), sig.end());
		const bool s0 = sig[0] & 1;
		for (i64 g = 0; g < P.m0; g++) {
			if (!live[g]) continue;
			u64 *G = F(g);
			std::fill(u.begin(), u.end(), 0);
			bool any_u = false;
			if (quad[g]) {
				for (i64 w = 0; w < W; w++) { u[w] = G[a * W + w]; G[a * W + w] = 0; }
				for (i64 b = 1; b < a; b++) if (qbit(&G[b * W], a)) { qflip(&G[b * W], a); qflip(u.data(), b); }
				any_u = !qzero(u.data(), W);
			}
			const bool la = qbit(G, a);
			if (la) { qflip(G, a); qxor(G, sig.data(), W); }
			if (any_u) {
				if (s0) qxor(G, u.data(), W);
				for (i64 w = 0; w < W; w++) { su[w] = sig[w] & u[w]; G[w] ^= su[w]; }
				for (i64 e = 1; e <= r; e++) {
					if (qbit(sig.data(), e)) qxor_above(&G[e * W], u.data(), e, W);
					if (qbit(u.data(), e)) qxor_above(&G[e * W], sig.data(), e, W);
				}
			}
			if (!la && !any_u) continue;
			if (!classify(g)) { P.inconsistent = true; break; }
		}
		f = -1;                                    // rescan: a substitution may have made earlier forms affine
	}
	if (P.inconsistent) {
		P.reff = 0; P.fw = 1; P.m = 1; P.forms.assign(1, 1);
		return;
	}
	P.alive.clear();
	for (i64 a = 1; a <= r; a++) if (var_alive[a]) P.alive.push_back((int)a);
	const i64 re = (i64)P.alive.size();
	P.reff = re;
	P.fw = (1 + re + re * (re - 1) / 2 + 63) / 64;
	P.m = 0;
	for (i64 f = 0; f < P.m0; f++) if (live[f]) P.m++;
	P.forms.assign((size_t)(std::max<i64>(P.m, 1) * P.fw), 0);
	i64 k = 0;
	for (i64 f = 0; f < P.m0; f++) {
		if (!live[f]) continue;
		const u64 *G = F(f);
		u64 *o = &P.forms[k++ * P.fw];
		if (G[0] & 1) o[0] |= 1;
		for (i64 v = 0; v < re; v++) {
			if (qbit(G, P.alive[v])) qflip(o, 1 + v);
			const u64 *row = &G[(i64)P.alive[v] * W];
			for (i64 v2 = v + 1; v2 < re; v2++)
				if (qbit(row, P.alive[v2])) qflip(o, 1 + re + v2 * (v2 - 1) / 2 + v);
		}
	}
}

// the point of the space that effective assignment y (reff bits) extends to; c_orig: its coefficients (dw words)
bool quad_point(const QuadPlan &P, const u64 *y, u64 *x, u64 *c_orig)
{
	const i64 r = P.r, W = P.W, words = P.words;
	std::vector<u64> c((size_t)W, 0);
	c[0] = 1;
	for (i64 v = 0; v < P.reff; v++) if (qbit(y, v)) qflip(c.data(), P.alive[v]);
	for (i64 k = (i64)P.sub_var.size() - 1; k >= 0; k--) {
		const u64 *sg = &P.sub_sigma[k * W];
		u64 par = 0;
		for (i64 w = 0; w < W; w++) par ^= sg[w] & c[w];
		if (__builtin_popcountll(par) & 1) qflip(c.data(), P.sub_var[k]);
	}
	std::copy(P.origin.begin(), P.origin.end(), x);
	std::fill(c_orig, c_orig + P.dw, 0);
	for (i64 a = 0; a < r; a++)
		if (qbit(c.data(), a + 1)) { qxor(x, &P.V[a * words], words); qxor(c_orig, &P.T[a * P.dw], P.dw); }
	for (size_t k = 0; k < P.kpiv.size(); k++) {
		const i64 s = P.kpiv[k];
		const bool v = (qbit(x, P.pair_i[s]) & qbit(x, P.pair_j[s])) ^ qbit(x, P.n + s);
		if (v) { qxor(x, &P.V[(r + (i64)k) * words], words); qxor(c_orig, &P.T[(r + (i64)k) * P.dw], P.dw); }
	}
	for (i64 s = 0; s < P.S; s++)                  // every product coordinate must now be the product of its linear bits
		if ((qbit(x, P.pair_i[s]) & qbit(x, P.pair_j[s])) != qbit(x, P.n + s)) return false;
	return true;
}

// a host vector into a buffer of the holder, on the holder's stream
template <class T>
hipError_t upload(Held &H, T **d, const std::vector<T> &h)
{
	const hipError_t e = H.get((void **)d, h.size() * sizeof(T));
	return e != hipSuccess ? e : hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, H.st);
}

int quad_forms_device(QuadPlan &P, int device, hipStream_t st)
{
	const i64 r = P.r, W = P.W, cells = (r + 1) * W;
	P.M.assign((size_t)(std::max<i64>(P.m0, 1) * cells), 0);
	if (P.m0 == 0) return GF2BV_OK;
	Held H(device, st);
	u64 *dl, *dq, *dout;
	int *dpi, *dpj, *dsi;
	i64 *dso;
	HIPCHK(upload(H, &dl, P.lin)); HIPCHK(upload(H, &dq, P.qaff));
	HIPCHK(upload(H, &dpi, P.pair_i)); HIPCHK(upload(H, &dpj, P.pair_j));
	HIPCHK(upload(H, &dso, P.sup_off)); HIPCHK(upload(H, &dsi, P.sup_idx));
	HIPCHK(H.get((void **)&dout, P.M.size() * 8));
	k_quad_forms<<<dim3((unsigned)P.m0), dim3(256), (size_t)cells * 8, st>>>(dl, dq, dpi, dpj, dso, dsi, (int)r, (int)W, dout);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(P.M.data(), dout, P.M.size() * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return GF2BV_OK;
}

// the first 64 forms (fw words each) that are linearly independent, in their order
std::vector<i64> first_independent_forms(const u64 *forms, i64 m, i64 fw)
{
	std::vector<i64> chosen;
	std::vector<u64> red;                          // reduced chosen forms, each with its pivot bit
	std::vector<i64> piv;
	std::vector<u64> v((size_t)fw);
	for (i64 f = 0; f < m && (i64)chosen.size() < 64; f++) {
		std::copy(forms + f * fw, forms + (f + 1) * fw, v.begin());
		for (size_t k = 0; k < piv.size(); k++) if (qbit(v.data(), piv[k])) qxor(v.data(), &red[k * fw], fw);
		i64 p = -1;
		for (i64 w = 0; w < fw && p < 0; w++) if (v[w]) p = w * 64 + __builtin_ctzll(v[w]);
		if (p < 0) continue;
		for (size_t k = 0; k < piv.size(); k++) if (qbit(&red[k * fw], p)) qxor(&red[k * fw], v.data(), fw);
		red.insert(red.end(), v.begin(), v.end());
		piv.push_back(p);
		chosen.push_back(f);
	}
	return chosen;
}

// The two-pass search of a degree, which supplies what really differs (SearchPasses): `tab`, the forms of the first pass bit-sliced
// for its search kernel; `E`, the mE forms the second pass tests, in its check kernel's layout; the two kernels and the search
// kernel's launch shape.  `total` counts every common zero, `ys` holds them when there are at most kQuadMaxPoints (in no particular order)
using SearchKernel = void (*)(const u64 *, int, int, u64, u64 *, u64, unsigned long long *, const u64 *, i64);
using CheckKernel = void (*)(const u64 *, i64, int, const u64 *, u64, u64 *, u64, unsigned long long *);
struct SearchPasses {
	const std::vector<u64> &tab, &E;
	i64 mE;
	SearchKernel search;
	CheckKernel check;
	int R, L;                                      // variables, and how many of them a lane walks
	unsigned block;
	size_t lds;
	QuadTimes &times;
};

// no form: the whole cube
void search_whole_cube(int R, std::vector<u64> &ys, u64 *total)
{
	*total = 1ull << R;
	if ((i64)*total <= kQuadMaxPoints) for (u64 y = 0; y < *total; y++) ys.push_back(y);
}

int search_two_pass(const SearchPasses &s, int device, hipStream_t st, std::vector<u64> &ys, u64 *total)
{
	static_assert(kQuadMaxCand == kQuadMaxPoints, "the candidate list doubles as the list of zeros");
	const int R = s.R, L = s.L;
	const u64 nlanes = 1ull << (R - L);
	const dim3 grid((unsigned)((nlanes + s.block - 1) / s.block)), block(s.block);
	const u64 ocap = (u64)kQuadMaxPoints, cap = (u64)kQuadMaxCand;
	Held H(device, st);
	u64 *dtab, *dE, *dcand, *dout;
	unsigned long long *dcnt;
	HIPCHK(upload(H, &dtab, s.tab)); HIPCHK(upload(H, &dE, s.E));
	HIPCHK(H.get((void **)&dcnt, 16));
	HIPCHK(hipMemsetAsync(dcnt, 0, 16, st));
	HIPCHK(H.get((void **)&dcand, cap * 8));
	HIPCHK(H.get((void **)&dout, ocap * 8));
	s.search<<<grid, block, s.lds, st>>>(dtab, R, L, nlanes, dcand, cap, dcnt, nullptr, 0);
	HIPCHK(hipGetLastError());
	u64 cnt[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(cnt, dcnt, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	s.times.candidates += (i64)cnt[0];
	const void *found = dout;
	if (s.mE == 0) {
		cnt[1] = cnt[0];                           // every form was in the first pass: its candidates are the zeros (cap == ocap)
		found = dcand;
	} else if (cnt[0] > cap) {
		// more candidates than can be kept: search again, each lane testing its candidates against the forms of E itself
		s.search<<<grid, block, s.lds, st>>>(dtab, R, L, nlanes, dout, ocap, dcnt + 1, dE, s.mE);
		HIPCHK(hipGetLastError());
	} else if (cnt[0]) {
		const u64 waves = std::min<u64>(cnt[0], 8192);
		s.check<<<dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st>>>(dE, s.mE, R, dcand, cnt[0], dout, ocap, dcnt + 1);
		HIPCHK(hipGetLastError());
	}
	if (s.mE) {
		HIPCHK(hipMemcpyAsync(cnt + 1, dcnt + 1, 8, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
	}
	*total = cnt[1];
	if ((i64)cnt[1] <= kQuadMaxPoints) {
		ys.resize((size_t)cnt[1]);
		if (cnt[1]) HIPCHK(hipMemcpyAsync(ys.data(), found, cnt[1] * 8, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
	}
	return GF2BV_OK;
}

// every common zero of m forms (equation-int layout, fw words) in R <= kQuadMaxEnum variables (total, ys: search_two_pass).  Every
// form goes into E, so the driver's branch for an empty E is never taken here
int quad_search_device(const u64 *forms, i64 m, i64 fw, int R, int device, hipStream_t st, std::vector<u64> &ys, u64 *total)
{
	ys.clear();
	if (m == 0) { search_whole_cube(R, ys, total); return GF2BV_OK; }
	auto coef = [&](i64 f, i64 bit) { return qbit(forms + f * fw, bit); };
	auto pair_bit = [&](i64 j, i64 k) { return 1 + R + (k > j ? k * (k - 1) / 2 + j : j * (j - 1) / 2 + k); };
	// the 64 forms of the first pass: the first that are linearly independent (a form in the span of those already chosen
	// removes no candidate, and leading forms of low rank are common -- pair coordinates over few variables come first)
	const std::vector<i64> chosen = first_independent_forms(forms, m, fw);
	std::vector<u64> tab((size_t)(1 + R + R * R), 0), E((size_t)(m * (R + 2)), 0);
	for (i64 f = 0; f < m; f++) {                  // every form in k_forms_check<2>'s layout
		u64 *e = &E[f * (R + 2)];
		if (coef(f, 0)) e[0] = 1;
		for (i64 k = 0; k < R; k++) {
			if (coef(f, 1 + k)) e[1] |= 1ull << k;
			for (i64 j = 0; j < k; j++) if (coef(f, pair_bit(j, k))) e[2 + j] |= 1ull << k;
		}
	}
	for (size_t c = 0; c < chosen.size(); c++) {   // the chosen ones bit-sliced: bit c of every word
		const i64 f = chosen[c];
		const u64 fb = 1ull << c;
		if (coef(f, 0)) tab[0] |= fb;
		for (i64 k = 0; k < R; k++) {
			if (coef(f, 1 + k)) tab[1 + k] |= fb;
			for (i64 j = 0; j < k; j++)
				if (coef(f, pair_bit(j, k))) { tab[1 + R + j * R + k] |= fb; tab[1 + R + k * R + j] |= fb; }
		}
	}
	const int H = std::max(0, std::min(R - 10, 18)), L = R - H;
	const unsigned bd = (unsigned)std::min<u64>(256, ((1ull << H) + 63) / 64 * 64);
	return search_two_pass({ tab, E, m, k_quad_search, k_forms_check<2>, R, L, bd, (size_t)bd * L * 8, g_quad_times }, device, st, ys, total);
}

int quad_plan_build(QuadPlan &P, const u64 *origin, const u64 *basis, i64 d, i64 words, i64 n, int device, hipStream_t st)
{
	auto t0 = std::chrono::steady_clock::now();
	quad_reduce(P, origin, basis, d, words, n, n * (n - 1) / 2);
	if (P.r > kQuadMaxRank) { P.reff = -1; g_quad_times.reduce += ms_since(t0); return GF2BV_OK; }
	quad_inputs(P);
	g_quad_times.reduce += ms_since(t0);
	t0 = std::chrono::steady_clock::now();
	if (device < 0) quad_forms_host(P);
	else { int rc = quad_forms_device(P, device, st); if (rc) return rc; }
	g_quad_times.forms += ms_since(t0);
	t0 = std::chrono::steady_clock::now();
	quad_affine(P);
	g_quad_times.affine += ms_since(t0);
	return GF2BV_OK;
}

// every consistent point of one space (words each, in no particular order) and its coefficients in the space's basis
// (coef: dw = ceil(d / 64) words each).  *total: their number (exact, also when
// `pts` could not hold them: more than kQuadMaxPoints); *gave_up: the search found no way down (step 3).
int quad_collect(const u64 *origin, const u64 *basis, i64 d, i64 words, i64 n, int max_enum, int device, hipStream_t st,
                 i64 parent_reff, int depth, std::vector<u64> &pts, std::vector<u64> &coef, u64 *total, i64 *lin_rank,
                 bool *gave_up)
{
	pts.clear(); coef.clear(); *total = 0;
	g_quad_times.levels = std::max<i64>(g_quad_times.levels, depth + 1);
	QuadPlan P;
	int rc = quad_plan_build(P, origin, basis, d, words, n, device, st);
	if (rc) return rc;
	if (depth == 0) *lin_rank = P.r;
	if (P.reff < 0) { *gave_up = true; return GF2BV_OK; }
	if (P.inconsistent) return GF2BV_OK;
	std::vector<u64> ys;                           // effective assignments, yw words each
	const i64 yw = std::max<i64>(1, (P.reff + 63) / 64);
	if (P.reff <= max_enum) {
		auto t0 = std::chrono::steady_clock::now();
		rc = quad_search_device(P.forms.data(), P.m, P.fw, (int)P.reff, device, st, ys, total);
		g_quad_times.search += ms_since(t0);
		if (rc) return rc;
	} else {
		if ((depth > 0 && P.reff >= parent_reff) || depth >= kQuadMaxDepth) { *gave_up = true; return GF2BV_OK; }
		// relinearise: the forms are the equations of a QuadraticSystem of reff unknowns; in augmented words the constant
		// (bit 0 of an equation int) is column `cols` and unknown k is column k
		auto t0 = std::chrono::steady_clock::now();
		const i64 cols = P.reff + P.reff * (P.reff - 1) / 2, rows = std::max(cols, P.m), stride = P.fw;
		std::vector<u64> aug((size_t)(rows * stride), 0);
		for (i64 f = 0; f < P.m; f++) {
			const u64 *e = &P.forms[f * P.fw];
			u64 *a = &aug[f * stride];
			for (i64 w = 0; w < stride; w++) a[w] = (e[w] >> 1) | (w + 1 < P.fw ? e[w + 1] << 63 : 0);
			if (e[0] & 1) qflip(a, cols);
		}
		gf2bv_result *res = nullptr;
		rc = gf2bv_solve_words(reinterpret_cast<const uint64_t *>(aug.data()), rows, cols, stride, GF2BV_MODE_AFFINE_SPACE, device, &res);
		if (rc) return rc;
		std::unique_ptr<gf2bv_result, void (*)(gf2bv_result *)> keep(res, gf2bv_result_free);
		g_quad_times.relin += ms_since(t0);
		if (gf2bv_result_status(res) != GF2BV_STATUS_SOLVED) return GF2BV_OK;
		const i64 d2 = gf2bv_result_dimension(res), w2 = gf2bv_result_words(res);
		std::vector<u64> o2((size_t)w2), b2((size_t)std::max<i64>(1, d2 * w2));
		gf2bv_result_origin(res, reinterpret_cast<uint64_t *>(o2.data()));
		if (d2) gf2bv_result_basis(res, reinterpret_cast<uint64_t *>(b2.data()));
		std::vector<u64> sub, sub_coef;
		i64 lr;
		rc = quad_collect(o2.data(), b2.data(), d2, w2, P.reff, max_enum, device, st, P.reff, depth + 1, sub, sub_coef, total, &lr, gave_up);
		if (rc || *gave_up) return rc;
		const i64 np = (i64)sub.size() / std::max<i64>(1, w2);
		ys.assign((size_t)(np * yw), 0);
		for (i64 k = 0; k < np; k++)
			for (i64 v = 0; v < P.reff; v++) if (qbit(&sub[k * w2], v)) qflip(&ys[k * yw], v);
	}
	if ((i64)*total > kQuadMaxPoints) return GF2BV_OK;
	const i64 np = (i64)ys.size() / yw;
	pts.assign((size_t)(np * words), 0);
	coef.assign((size_t)(np * P.dw), 0);
	for (i64 k = 0; k < np; k++)
		if (!quad_point(P, &ys[k * yw], &pts[k * words], &coef[k * P.dw]))
			return fail(GF2BV_ERR_HIP, "quad search: a point that passed the forms is not consistent (internal error)");
	return GF2BV_OK;
}

// what gf2bv_quad_plan and gf2bv_quad_plan_device hand out of a built plan
void quad_plan_export(const QuadPlan &P, int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms, int64_t forms_cap)
{
	*r = P.r; *r_eff = P.reff;
	*m = P.reff < 0 ? 0 : P.m;
	*form_words = P.reff < 0 ? 0 : P.fw;
	if (forms && P.reff >= 0 && P.m <= forms_cap) std::copy(P.forms.begin(), P.forms.begin() + P.m * P.fw, reinterpret_cast<u64 *>(forms));
}

// What gf2bv_quad_search_alloc and gf2bv_cubic_search_alloc do once their arguments are checked: the pool stream, `collect` (every
// consistent point with its coefficients in the space's basis), AffineSpace order, the first max_solutions points in a malloc'ed buffer
// (collect: int(hipStream_t, std::vector<u64> &pts, std::vector<u64> &coef, u64 *total, bool *gave_up))
template <class Collect>
int search_alloc(QuadTimes &times, int64_t dimension, int64_t words, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank,
                 uint64_t **out_words, Collect &&collect)
{
	*count = 0; *lin_rank = 0; *out_words = nullptr;
	int rc = check_device(device);
	if (rc) return rc;
	times = QuadTimes();
	const auto t0 = std::chrono::steady_clock::now();
	Held H(device);
	HIPCHK(H.stream(0));
	std::vector<u64> pts, coef;
	u64 total = 0;
	bool gave_up = false;
	rc = collect(H.st, pts, coef, &total, &gave_up);
	times.total = ms_since(t0);
	if (rc) return rc;
	if (gave_up) { *count = -1; return GF2BV_OK; }
	*count = (int64_t)total;
	if ((i64)total > kQuadMaxPoints) {
		if (max_solutions > 0) return fail(GF2BV_ERR_NOMEM, "more than 2^22 consistent points: too many to collect and order");
		return GF2BV_OK;
	}
	// iteration order of AffineSpace: the Gray walk for dimension <= 64 (inverse-Gray index of the coefficients), the
	// binary walk above (the coefficients as an integer, basis[0] the least significant bit)
	const i64 np = (i64)total, dw = std::max<i64>(1, (dimension + 63) / 64);
	std::vector<i64> order((size_t)np);
	for (i64 k = 0; k < np; k++) order[k] = k;
	if (dimension <= 64) {
		std::vector<u64> key((size_t)np);
		for (i64 k = 0; k < np; k++) {
			u64 g = coef[k * dw];
			for (int sh = 1; sh < 64; sh <<= 1) g ^= g >> sh;
			key[k] = g;
		}
		std::sort(order.begin(), order.end(), [&](i64 a, i64 b) { return key[a] < key[b]; });
	} else {
		std::sort(order.begin(), order.end(), [&](i64 a, i64 b) {
			for (i64 w = dw - 1; w >= 0; w--)
				if (coef[a * dw + w] != coef[b * dw + w]) return coef[a * dw + w] < coef[b * dw + w];
			return false;
		});
	}
	const i64 nout = std::min<i64>(np, max_solutions);
	if (nout == 0) return GF2BV_OK;
	uint64_t *out = static_cast<uint64_t *>(malloc(sizeof(uint64_t) * (size_t)(nout * words)));
	if (!out) return fail(GF2BV_ERR_NOMEM, "out of host memory");
	for (i64 k = 0; k < nout; k++) memcpy(out + k * words, &pts[order[k] * words], sizeof(uint64_t) * (size_t)words);
	*out_words = out;
	return GF2BV_OK;
}

}  // namespace

// ---- cubic and quartic search: the consistent points of a solution space over the columns of degree A = 3, 4 ---------------------
//   A space x(c) = o ^ B c over n linear coordinates followed by the product coordinates of 2 .. A members:
// C(n,2) pairs, C(n,3) triples (the columns of degree-3 XL and of PackedCubicSystem) and at A = 4 the C(n,4) quadruples (the columns of
// degree-4 XL and of PackedQuarticSystem).  Step 1 is the quadratic search's with N = cols (quad_reduce, quad_inputs).  Step 2: one
// form of degree A in r variables per product coordinate outside P (k_forms_products<A>, k_forms_sum).  Affine forms are eliminated by
// re-parametrising: they are solved as a linear system, c_a = c_0 ^ G y over the free variables y, the affine inputs are composed with
// that map and the forms rebuilt in fewer variables, until no affine form appears.  Step 3: r_eff <= max_enum: the degree's search
// kernel (k_cubic_search, k_quartic_search) + k_forms_check<A>; above: the search gives up (there is no relinearisation level).
// A degree is described once, by FormsDegree<A> below the bodies, which take it as their template parameter D.
namespace {

constexpr i64 kFormsMaxRank = 64;               // larger projection ranks are not reduced (a point of the forms is one word)
constexpr i64 kFormsBytes = 1ll << 30;          // what the forms of one build (products and forms) or of one search may take
constexpr int kFormsMaxEnum = 40;
constexpr int kCubicWalk = 12;                  // low variables a lane of k_cubic_search walks (78 words of LDS a lane)
constexpr int kQuarticWalk = 12;                // ... and of k_quartic_search (298 words of LDS a lane, 149 KiB a workgroup)
constexpr int kMaxArity = 4;                     // the highest degree: what a Monomial holds

thread_local QuadTimes g_cubic_times, g_quartic_times;

// The layout of a form, of a space's columns and of the kernels' tables: the monomials in blocks by size, a monomial with members
// m_0 < m_1 < ... at its block's start + SUM_t C(m_t, t + 1).  Every size below is a sum of binomials over a range of monomial sizes
constexpr i64 binom(i64 h, int t)
{
	i64 c = 1;
	for (int k = 1; k <= t; k++) c = c * (h - k + 1) / k;
	return c;
}
constexpr i64 binom_sum(i64 h, int lo, int hi)  // SUM_{t = lo .. hi} C(h, t); block `size` of a form over R variables starts at (R, 0, size - 1)
{
	i64 s = 0;
	for (int t = lo; t <= hi; t++) s += binom(h, t);
	return s;
}
using Monomial = std::array<int, kMaxArity>;    // the members, largest first, -1 behind them
i64 monomial_bit(i64 R, const Monomial &mm)     // its bit in a form over R variables
{
	int size = 0;
	while (size < kMaxArity && mm[size] >= 0) size++;
	i64 q = binom_sum(R, 0, size - 1);
	for (int i = 0; i < size; i++) q += binom(mm[i], size - i);
	return q;
}
// the monomials of `size` members over R variables in layout order: fn(the monomial, its place in the block)
template <class Fn>
void each_monomial(i64 R, int size, Fn fn)
{
	if (size > R) return;
	Monomial mm;
	mm.fill(-1);
	for (int i = 0; i < size; i++) mm[i] = size - 1 - i;
	for (i64 at = 0;; at++) {
		fn(mm, at);
		int i = size - 1;                           // the smallest member steps; one that reaches the member above starts again, and that one steps
		while (i >= 0 && ++mm[i] == (i ? mm[i - 1] : (int)R)) { mm[i] = size - 1 - i; i--; }
		if (i < 0) return;
	}
}

struct CubicPlan : QuadPlan {                    // the plan of either degree (lin, qaff: the affine inputs in the R variables left; M unused)
	explicit CubicPlan(int arity_) : arity(arity_) {}
	const int arity;                             // members of a product coordinate at most: the degree's (FormsDegree<A>::plan)
	std::vector<int> mem;                        // S x arity: the members of a product coordinate, -1 where it has fewer
	std::vector<u64> lin0, qaff0;                // the affine inputs in the r coefficients c_a
	std::vector<u64> amap;                       // r x W: c_a as an affine form in the R variables left (bit 0 constant, bit 1 + v)
	i64 R = 0, rounds = 0;
};

using ProductsKernel = void (*)(const u64 *, const u64 *, const int *, int, int, int, u64 *);

void cubic_reduce(CubicPlan &P, const u64 *origin, const u64 *basis, i64 d, i64 words, i64 n)
{
	const int arity = P.arity;
	quad_reduce(P, origin, basis, d, words, n, binom_sum(n, 2, arity));
	if (P.r > kFormsMaxRank) return;
	quad_inputs(P);
	P.lin0.swap(P.lin); P.qaff0.swap(P.qaff);
	P.lin.assign(P.lin0.size(), 0); P.qaff.assign(P.qaff0.size(), 0);
	P.mem.assign((size_t)(arity * std::max<i64>(P.S, 1)), -1);
	i64 s = 0;
	for (int size = 2; size <= arity; size++)
		each_monomial(n, size, [&](const Monomial &mm, i64) { std::copy(mm.begin(), mm.begin() + size, &P.mem[arity * s++]); });
	P.R = P.r;
	P.amap.assign((size_t)(std::max<i64>(P.r, 1) * P.W), 0);
	for (i64 a = 0; a < P.r; a++) qflip(&P.amap[a * P.W], a + 1);
}

// an affine form in the c_a composed with amap
void cubic_compose_form(const CubicPlan &P, const u64 *f, u64 *o)
{
	std::fill(o, o + P.W, 0);
	if (f[0] & 1) o[0] = 1;
	for (i64 a = 1; a <= P.r; a++) if (qbit(f, a)) qxor(o, &P.amap[(a - 1) * P.W], P.W);
}
void cubic_compose(CubicPlan &P)
{
	for (i64 i = 0; i < P.n; i++) cubic_compose_form(P, &P.lin0[i * P.W], &P.lin[i * P.W]);
	for (i64 s = 0; s < P.S; s++) cubic_compose_form(P, &P.qaff0[s * P.W], &P.qaff[s * P.W]);
}

// the host twin of k_forms_products<A> + k_forms_sum at the plan's arity (gf2bv_*_plan never touches a device): polynomial
// multiplication, monomial by monomial, through a decode table of the layout
void cubic_forms_host(const CubicPlan &P, i64 fw, std::vector<u64> &F)
{
	const int ar = P.arity;
	const i64 R = P.R, W = P.W;
	std::vector<Monomial> dec((size_t)binom_sum(R, 0, ar));
	for (int size = 0; size <= ar; size++)
		each_monomial(R, size, [&](const Monomial &mm, i64 at) { dec[binom_sum(R, 0, size - 1) + at] = mm; });
	auto with = [&](Monomial mm, int v) -> i64 {               // the bit of the monomial mm times x_v; mm has at most arity - 1 members
		                                                           // (a product of fewer than arity forms), so its last slot is free
		if (std::find(mm.begin(), mm.end(), v) == mm.end()) { mm[kMaxArity - 1] = v; std::sort(mm.begin(), mm.end(), std::greater<int>()); }
		return monomial_bit(R, mm);
	};
	auto mul = [&](const std::vector<u64> &f, const u64 *aff, std::vector<u64> &out) {      // f of degree <= 2 times an affine form
		std::fill(out.begin(), out.end(), 0);
		for (i64 w = 0; w < fw; w++)
			for (u64 bits = f[w]; bits; bits &= bits - 1) {
				const i64 q = w * 64 + __builtin_ctzll(bits);
				if (aff[0] & 1) qflip(out.data(), q);
				for (i64 v = 0; v < R; v++) if (qbit(aff, v + 1)) qflip(out.data(), with(dec[q], (int)v));
			}
	};
	std::vector<u64> V((size_t)(std::max<i64>(P.S, 1) * fw), 0), a((size_t)fw), b((size_t)fw);
	for (i64 s = 0; s < P.S; s++) {
		std::fill(a.begin(), a.end(), 0);
		std::copy(&P.lin[(i64)P.mem[ar * s] * W], &P.lin[(i64)P.mem[ar * s] * W] + std::min(W, fw), a.begin());
		mul(a, &P.lin[(i64)P.mem[ar * s + 1] * W], b);
		for (int f = 2; f < ar && P.mem[ar * s + f] >= 0; f++) { mul(b, &P.lin[(i64)P.mem[ar * s + f] * W], a); a.swap(b); }
		qxor(b.data(), &P.qaff[s * W], std::min(W, fw));
		std::copy(b.begin(), b.end(), &V[s * fw]);
	}
	F.assign((size_t)(std::max<i64>(P.m0, 1) * fw), 0);
	for (i64 t = 0; t < P.m0; t++)
		for (i64 k = P.sup_off[t]; k < P.sup_off[t + 1]; k++) qxor(&F[t * fw], &V[(i64)P.sup_idx[k] * fw], fw);
}

int cubic_forms_device(const CubicPlan &P, ProductsKernel products, i64 fw, std::vector<u64> &F, int device, hipStream_t st)
{
	F.assign((size_t)(std::max<i64>(P.m0, 1) * fw), 0);
	if (P.m0 == 0) return GF2BV_OK;
	Held H(device, st);
	u64 *dl, *dq, *dv, *dout;
	int *dm, *dsi;
	i64 *dso;
	HIPCHK(upload(H, &dl, P.lin)); HIPCHK(upload(H, &dq, P.qaff)); HIPCHK(upload(H, &dm, P.mem));
	HIPCHK(upload(H, &dso, P.sup_off)); HIPCHK(upload(H, &dsi, P.sup_idx));
	HIPCHK(H.get((void **)&dv, (size_t)(P.S * fw) * 8)); HIPCHK(H.get((void **)&dout, (size_t)(P.m0 * fw) * 8));
	products<<<dim3((unsigned)P.S), dim3(256), 0, st>>>(dl, dq, dm, (int)P.R, (int)P.W, (int)fw, dv);
	HIPCHK(hipGetLastError());
	k_forms_sum<<<dim3((unsigned)P.m0), dim3(256), 0, st>>>(dv, dso, dsi, (int)fw, dout);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(F.data(), dout, (size_t)(P.m0 * fw) * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return GF2BV_OK;
}

// One round of the affine elimination: the affine forms among F (m0 x fw, R variables) solved as a linear system and amap composed with
// its solution.  false: no affine form but zeros (nothing changed).  P.inconsistent: the system has no solution.
bool cubic_affine_round(CubicPlan &P, i64 fw, const std::vector<u64> &F)
{
	const i64 R = P.R, W = P.W, aw = std::min(W, fw), w0 = (R + 1) >> 6;
	std::vector<u64> rows, v((size_t)W);                   // reduced affine forms, each with its pivot variable's bit
	std::vector<i64> piv;
	for (i64 f = 0; f < P.m0; f++) {
		const u64 *e = &F[f * fw];
		bool affine = true;
		if (w0 < fw) {
			affine = (e[w0] >> ((R + 1) & 63)) == 0;
			for (i64 w = w0 + 1; w < fw && affine; w++) affine = e[w] == 0;
		}
		if (!affine) continue;
		std::fill(v.begin(), v.end(), 0);
		std::copy(e, e + aw, v.begin());
		for (size_t k = 0; k < piv.size(); k++) if (qbit(v.data(), piv[k])) qxor(v.data(), &rows[k * W], W);
		i64 p = -1;
		for (i64 w = 0; w < W && p < 0; w++) { const u64 x = v[w] & (w ? ~0ull : ~1ull); if (x) p = w * 64 + __builtin_ctzll(x); }
		if (p < 0) {
			if (v[0] & 1) { P.inconsistent = true; return true; }
			continue;
		}
		for (size_t k = 0; k < piv.size(); k++) if (qbit(&rows[k * W], p)) qxor(&rows[k * W], v.data(), W);
		rows.insert(rows.end(), v.begin(), v.end());
		piv.push_back(p);
	}
	if (piv.empty()) return false;
	std::vector<i64> row_of((size_t)(R + 1), -1), fresh((size_t)(R + 1), -1);
	for (size_t k = 0; k < piv.size(); k++) row_of[piv[k]] = (i64)k;
	i64 nr = 0;
	for (i64 b = 1; b <= R; b++) if (row_of[b] < 0) fresh[b] = ++nr;              // bit of the free variable in the new forms
	std::vector<u64> sub((size_t)((R + 1) * W), 0);        // variable bit b as an affine form in the variables left
	for (i64 b = 1; b <= R; b++) {
		u64 *o = &sub[b * W];
		if (row_of[b] < 0) { qflip(o, fresh[b]); continue; }
		const u64 *e = &rows[row_of[b] * W];
		if (e[0] & 1) o[0] = 1;
		for (i64 c = 1; c <= R; c++) if (c != b && qbit(e, c)) qflip(o, fresh[c]);
	}
	std::vector<u64> next((size_t)(std::max<i64>(P.r, 1) * W), 0);
	for (i64 a = 0; a < P.r; a++) {
		const u64 *e = &P.amap[a * W];
		u64 *o = &next[a * W];
		if (e[0] & 1) o[0] = 1;
		for (i64 b = 1; b <= R; b++) if (qbit(e, b)) qxor(o, &sub[b * W], W);
	}
	P.amap.swap(next);
	P.R = nr;
	return true;
}

template <class D>
int forms_plan_build(CubicPlan &P, const u64 *origin, const u64 *basis, i64 d, i64 words, i64 n, int device, hipStream_t st)
{
	auto t0 = std::chrono::steady_clock::now();
	cubic_reduce(P, origin, basis, d, words, n);
	D::times().reduce += ms_since(t0);
	if (P.r > kFormsMaxRank) { P.reff = -1; return GF2BV_OK; }
	std::vector<u64> F;
	i64 fw = 1;
	for (;;) {
		t0 = std::chrono::steady_clock::now();
		cubic_compose(P);
		fw = (D::width(P.R) + 63) / 64;
		if ((P.S + P.m0) * fw * 8 > kFormsBytes) return fail(GF2BV_ERR_NOMEM, D::kNomemBuildText);
		if (device < 0) cubic_forms_host(P, fw, F);
		else { int rc = cubic_forms_device(P, D::kProducts, fw, F, device, st); if (rc) return rc; }
		D::times().forms += ms_since(t0);
		t0 = std::chrono::steady_clock::now();
		P.rounds++;
		const bool changed = cubic_affine_round(P, fw, F);
		D::times().affine += ms_since(t0);
		if (P.inconsistent) { P.reff = 0; P.fw = 1; P.m = 1; P.forms.assign(1, 1); return GF2BV_OK; }
		if (!changed) break;
	}
	P.reff = P.R; P.fw = fw; P.m = 0;
	P.forms.clear();
	for (i64 f = 0; f < P.m0; f++)
		if (!qzero(&F[f * fw], fw)) { P.forms.insert(P.forms.end(), &F[f * fw], &F[f * fw] + fw); P.m++; }
	if (P.forms.empty()) P.forms.assign((size_t)fw, 0);
	return GF2BV_OK;
}

// the point of the space that effective assignment y[0] (reff <= 64 bits) extends to; c_orig: its coefficients (dw words)
bool cubic_point(const CubicPlan &P, const u64 *y, u64 *x, u64 *c_orig)
{
	const i64 r = P.r, W = P.W, words = P.words;
	const u64 ye[2] = {1ull | (y[0] << 1), y[0] >> 63};
	std::copy(P.origin.begin(), P.origin.end(), x);
	std::fill(c_orig, c_orig + P.dw, 0);
	for (i64 a = 0; a < r; a++) {
		u64 par = 0;
		for (i64 w = 0; w < W; w++) par ^= P.amap[a * W + w] & ye[w];
		if (__builtin_popcountll(par) & 1) { qxor(x, &P.V[a * words], words); qxor(c_orig, &P.T[a * P.dw], P.dw); }
	}
	const int ar = P.arity;
	auto prod = [&](i64 s) {
		bool v = qbit(x, P.mem[ar * s]) & qbit(x, P.mem[ar * s + 1]);
		for (int f = 2; f < ar && P.mem[ar * s + f] >= 0; f++) v &= qbit(x, P.mem[ar * s + f]);
		return v;
	};
	for (size_t k = 0; k < P.kpiv.size(); k++) {
		const i64 s = P.kpiv[k];
		if (prod(s) != qbit(x, P.n + s)) { qxor(x, &P.V[(r + (i64)k) * words], words); qxor(c_orig, &P.T[(r + (i64)k) * P.dw], P.dw); }
	}
	for (i64 s = 0; s < P.S; s++) if (prod(s) != qbit(x, P.n + s)) return false;
	return true;
}

// every common zero of m forms of degree D::kArity (equation-int layout, fw words) in R <= kFormsMaxEnum variables (total, ys:
// search_two_pass).  Only the forms outside the first pass go into E: with none left the driver reads the candidates as the zeros
template <class D>
int forms_search_device(const u64 *forms, i64 m, i64 fw, int R, int device, hipStream_t st, std::vector<u64> &ys, u64 *total)
{
	ys.clear();
	if (m == 0) { search_whole_cube(R, ys, total); return GF2BV_OK; }
	const i64 nb = D::width(R), ew = D::check_words(R);
	if (m * ew * 8 > kFormsBytes) return fail(GF2BV_ERR_NOMEM, D::kNomemSearchText);
	const std::vector<i64> chosen = first_independent_forms(forms, m, fw);
	// the second pass tests the forms the first did not hold (a chosen form vanishes at every candidate; a zero form everywhere)
	std::vector<char> in_first((size_t)m, 0);
	for (i64 f : chosen) in_first[f] = 1;
	std::vector<i64> rest;
	for (i64 f = 0; f < m; f++) if (!in_first[f] && !qzero(forms + f * fw, fw)) rest.push_back(f);
	const i64 mr = (i64)rest.size();
	// where bit q of a form goes in k_forms_check's layout: the largest member of its monomial is the bit, and the word is 1 + the bit
	// of the other members' monomial, one size smaller (the constant: bit 0 of word 0).  Built once a call, and only when a form is left
	// for the second pass
	std::vector<std::pair<i64, int>> slot(mr ? (size_t)nb : 0, {0, 0});
	for (int size = 1; mr && size <= D::kArity; size++)
		each_monomial(R, size, [&](const Monomial &mm, i64 at) {
			Monomial others;
			others.fill(-1);
			std::copy(mm.begin() + 1, mm.end(), others.begin());
			slot[binom_sum(R, 0, size - 1) + at] = {1 + monomial_bit(R, others), mm[0]};
		});
	std::vector<u64> tab((size_t)nb, 0), E((size_t)(std::max<i64>(mr, 1) * ew), 0);
	for (i64 g = 0; g < mr; g++) {
		const u64 *src = forms + rest[g] * fw;
		for (i64 q = 0; q < nb; q++) if (qbit(src, q)) E[g * ew + slot[q].first] |= 1ull << slot[q].second;
	}
	for (size_t c = 0; c < chosen.size(); c++) {   // the chosen ones bit-sliced: bit c of every word; tab is indexed like a form's bits
		const u64 *src = forms + chosen[c] * fw;
		for (i64 q = 0; q < nb; q++) if (qbit(src, q)) tab[q] |= 1ull << c;
	}
	const int L = std::min(R, D::kWalk);
	constexpr size_t lds_max = (size_t)64 * 8 * D::state_words(D::kWalk);
	const size_t lds = (size_t)64 * 8 * D::state_words(L);
	if constexpr (lds_max > 65536) {               // (k_quartic_search only: 149 KiB at its full walk; raised once, to the kernel's maximum)
		static std::mutex mu;
		static std::map<int, bool> raised;         // device -> the > 64 KiB dynamic-LDS attribute has been raised there
		std::lock_guard<std::mutex> lk(mu);
		if (!raised[device]) {
			HIPCHK(hipFuncSetAttribute((const void *)D::kSearch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
			raised[device] = true;
		}
	}
	return search_two_pass({ tab, E, mr, D::kSearch, D::kCheck, R, L, 64, lds, D::times() }, device, st, ys, total);
}

// every consistent point of the space and its coefficients: quad_collect without the relinearisation level
template <class D>
int forms_collect(const u64 *origin, const u64 *basis, i64 d, i64 words, i64 n, int max_enum, int device, hipStream_t st,
                  std::vector<u64> &pts, std::vector<u64> &coef, u64 *total, i64 *lin_rank, bool *gave_up)
{
	pts.clear(); coef.clear(); *total = 0;
	CubicPlan P = D::plan();
	int rc = forms_plan_build<D>(P, origin, basis, d, words, n, device, st);
	D::times().levels = P.rounds;
	*lin_rank = P.r;
	if (rc) return rc;
	if (P.reff < 0 || (!P.inconsistent && P.reff > max_enum)) { *gave_up = true; return GF2BV_OK; }
	if (P.inconsistent) return GF2BV_OK;
	std::vector<u64> ys;
	auto t0 = std::chrono::steady_clock::now();
	rc = forms_search_device<D>(P.forms.data(), P.m, P.fw, (int)P.reff, device, st, ys, total);
	D::times().search += ms_since(t0);
	if (rc) return rc;
	if ((i64)*total > kQuadMaxPoints) return GF2BV_OK;
	const i64 np = (i64)ys.size();
	pts.assign((size_t)(np * words), 0);
	coef.assign((size_t)(np * P.dw), 0);
	for (i64 k = 0; k < np; k++)
		if (!cubic_point(P, &ys[k], &pts[k * words], &coef[k * P.dw])) return fail(GF2BV_ERR_HIP, D::kBadPointText);
	return GF2BV_OK;
}

// ---- what a degree is, once: the entries below and the bodies above take it as D ---------------------------------------------------
// Plan, plan(): the plan type and a fresh plan of the degree.  kArity: members of a product coordinate at most; the sizes follow from it (binom_sum): cols, the columns of a
// space over n linear coordinates, and width, the bits of a form over R variables.  kMaxLin, kLinText, kWordsText: the space check.
// kPointWords: the words of an assignment a point is read from, 0 for as many as cover r_eff bits.  build, point, search, collect:
// the plan build, the point function, the device search and the collection of every consistent point.  times: the QuadTimes it writes
struct QuadDegree {
	using Plan = QuadPlan;
	static Plan plan() { return Plan(); }
	static constexpr int kArity = 2, kMaxEnum = kQuadMaxEnum;
	static constexpr i64 kMaxLin = 46340, kPointWords = 0;
	static constexpr const char *kLinText = "n_lin must be 1..46340", *kWordsText = "words does not cover n_lin + n_lin(n_lin-1)/2 columns";
	static constexpr i64 cols(i64 n) { return binom_sum(n, 1, kArity); }
	static constexpr i64 width(i64 R) { return binom_sum(R, 0, kArity); }
	static QuadTimes &times() { return g_quad_times; }
	static constexpr auto build = quad_plan_build;
	static constexpr auto point = quad_point;
	static constexpr auto search = quad_search_device;
	static int collect(const u64 *origin, const u64 *basis, i64 d, i64 words, i64 n, int max_enum, int device, hipStream_t st,
	                   std::vector<u64> &pts, std::vector<u64> &coef, u64 *total, i64 *lin_rank, bool *gave_up)
	{
		return quad_collect(origin, basis, d, words, n, max_enum, device, st, 0, 0, pts, coef, total, lin_rank, gave_up);
	}
};
// Degrees 3 and 4 share their bodies (forms_plan_build, cubic_point, forms_search_device, forms_collect), so FormsDegree<A> computes
// what follows from A and FormsFacts<A> states the rest: the space check, the walk and its tuned search kernel, the times, the messages.
// state_words: words of LDS a lane of the search kernel keeps at a walk of L variables.  check_words: words of a form in k_forms_check's
// layout.  A further degree is a FormsFacts, kMaxArity raised to it, and a level in each of form_value, qs_c / qs_off / qs_root under
// k_forms_products and its search kernel
template <int A> struct FormsFacts;
template <> struct FormsFacts<3> {
	static constexpr i64 kMaxLin = 2000;
	static constexpr int kWalk = kCubicWalk;
	static constexpr SearchKernel kSearch = k_cubic_search;
	static QuadTimes &times() { return g_cubic_times; }
	static constexpr const char *kLinText = "n_lin must be 1..2000", *kWordsText = "words does not cover n_lin + C(n_lin,2) + C(n_lin,3) columns",
	                            *kNomemBuildText = "the cubic forms of this space take more than 1 GiB",
	                            *kNomemSearchText = "the cubic forms of this search take more than 1 GiB",
	                            *kBadPointText = "cubic search: a point that passed the forms is not consistent (internal error)";
};
template <> struct FormsFacts<4> {
	static constexpr i64 kMaxLin = 450;
	static constexpr int kWalk = kQuarticWalk;
	static constexpr SearchKernel kSearch = k_quartic_search;
	static QuadTimes &times() { return g_quartic_times; }
	static constexpr const char *kLinText = "n_lin must be 1..450",
	                            *kWordsText = "words does not cover n_lin + C(n_lin,2) + C(n_lin,3) + C(n_lin,4) columns",
	                            *kNomemBuildText = "the quartic forms of this space take more than 1 GiB",
	                            *kNomemSearchText = "the quartic forms of this search take more than 1 GiB",
	                            *kBadPointText = "quartic search: a point that passed the forms is not consistent (internal error)";
};
template <int A>
struct FormsDegree : FormsFacts<A> {
	static_assert(A >= 3 && A <= kMaxArity, "a Monomial holds kMaxArity members");
	using Plan = CubicPlan;
	static Plan plan() { return Plan(A); }
	static constexpr int kArity = A, kMaxEnum = kFormsMaxEnum;
	static constexpr i64 kPointWords = 1;
	static constexpr i64 cols(i64 n) { return binom_sum(n, 1, A); }
	static constexpr i64 width(i64 R) { return binom_sum(R, 0, A); }
	static constexpr i64 state_words(i64 L) { return binom_sum(L, 1, A - 1); }
	static constexpr i64 check_words(i64 R) { return 1 + binom_sum(R, 0, A - 1); }
	static constexpr ProductsKernel kProducts = k_forms_products<A>;
	static constexpr CheckKernel kCheck = k_forms_check<A>;
	static constexpr auto build = forms_plan_build<FormsDegree>;
	static constexpr auto point = cubic_point;
	static constexpr auto search = forms_search_device<FormsDegree>;
	static constexpr auto collect = forms_collect<FormsDegree>;
};
using CubicDegree = FormsDegree<3>;
using QuarticDegree = FormsDegree<4>;
static_assert((size_t)64 * 8 * QuarticDegree::state_words(kQuarticWalk) <= 160 * 1024, "the walk's state fits a CU's LDS");
static_assert(QuadDegree::kMaxEnum == 40 && CubicDegree::kMaxEnum == 40 && QuarticDegree::kMaxEnum == 40, "the entries' messages name 40");

template <class D>
int check_space(const u64 *origin, const u64 *basis, i64 d, i64 words, i64 n_lin)
{
	if (!origin || (d > 0 && !basis)) return fail(GF2BV_ERR_ARG, "null pointer");
	if (d < 0 || words <= 0) return fail(GF2BV_ERR_ARG, "dimension must be >= 0 and words > 0");
	if (n_lin < 1 || n_lin > D::kMaxLin) return fail(GF2BV_ERR_ARG, D::kLinText);
	if (words < (D::cols(n_lin) + 63) / 64) return fail(GF2BV_ERR_ARG, D::kWordsText);
	return GF2BV_OK;
}

// gf2bv_*_plan (device -1: the forms are built on the host) and gf2bv_*_plan_device
template <class D>
int search_plan(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin, bool on_device, int device,
                int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms_, int64_t forms_cap)
{
	const u64 *origin = reinterpret_cast<const u64 *>(origin_), *basis = reinterpret_cast<const u64 *>(basis_);
	int rc = check_space<D>(origin, basis, dimension, words, n_lin);
	if (rc) return rc;
	if (!r || !r_eff || !m || !form_words) return fail(GF2BV_ERR_ARG, "null pointer");
	Held H(device);
	if (on_device) {
		if ((rc = check_device(device))) return rc;
		HIPCHK(H.stream(0));
	}
	typename D::Plan P = D::plan();
	rc = D::build(P, origin, basis, dimension, words, n_lin, device, H.st);
	if (rc) return rc;
	quad_plan_export(P, r, r_eff, m, form_words, forms_, forms_cap);
	return GF2BV_OK;
}

template <class D>
int search_points(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin, const uint64_t *ys_,
                  int64_t nys, int64_t y_words, uint64_t *out_words_)
{
	const u64 *origin = reinterpret_cast<const u64 *>(origin_), *basis = reinterpret_cast<const u64 *>(basis_);
	const u64 *ys = reinterpret_cast<const u64 *>(ys_);
	u64 *out_words = reinterpret_cast<u64 *>(out_words_);
	int rc = check_space<D>(origin, basis, dimension, words, n_lin);
	if (rc) return rc;
	if (nys < 0 || (nys > 0 && (!ys || !out_words))) return fail(GF2BV_ERR_ARG, "null pointer");
	if (D::kPointWords && y_words < D::kPointWords) return fail(GF2BV_ERR_ARG, "y_words does not cover r_eff bits");
	typename D::Plan P = D::plan();
	rc = D::build(P, origin, basis, dimension, words, n_lin, -1, nullptr);
	if (rc) return rc;
	if (P.reff < 0 || P.inconsistent) return fail(GF2BV_ERR_ARG, "the space has no forms to map from");
	if (!D::kPointWords && y_words < std::max<i64>(1, (P.reff + 63) / 64)) return fail(GF2BV_ERR_ARG, "y_words does not cover r_eff bits");
	std::vector<u64> c((size_t)P.dw);
	for (i64 k = 0; k < nys; k++)
		if (!D::point(P, ys + k * y_words, out_words + k * words, c.data()))
			return fail(GF2BV_ERR_ARG, "an assignment that is not a common zero of the forms");
	return GF2BV_OK;
}

template <class D>
int search_forms(const uint64_t *forms_, int64_t m, int64_t r_eff, int device, int64_t max_out, int64_t *count, uint64_t *out_)
{
	const u64 *forms = reinterpret_cast<const u64 *>(forms_);
	u64 *out = reinterpret_cast<u64 *>(out_);
	if (!count || (m > 0 && !forms) || (max_out > 0 && !out) || m < 0 || max_out < 0) return fail(GF2BV_ERR_ARG, "null pointer");
	if (r_eff < 0 || r_eff > D::kMaxEnum) return fail(GF2BV_ERR_ARG, "r_eff must be 0..40");
	*count = 0;
	int rc = check_device(device);
	if (rc) return rc;
	Held H(device);
	HIPCHK(H.stream(0));
	std::vector<u64> ys;
	u64 total = 0;
	rc = D::search(forms, m, (D::width(r_eff) + 63) / 64, (int)r_eff, device, H.st, ys, &total);
	if (rc) return rc;
	*count = (int64_t)total;
	if ((i64)total > kQuadMaxPoints && max_out > 0) return fail(GF2BV_ERR_NOMEM, "more common zeros than can be collected");
	std::sort(ys.begin(), ys.end());
	std::copy(ys.begin(), ys.begin() + std::min<i64>((i64)ys.size(), max_out), out);
	return GF2BV_OK;
}

template <class D>
int search_space_alloc(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin, int max_enum,
                       int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t **out_words)
{
	const u64 *origin = reinterpret_cast<const u64 *>(origin_), *basis = reinterpret_cast<const u64 *>(basis_);
	int rc = check_space<D>(origin, basis, dimension, words, n_lin);
	if (rc) return rc;
	if (!count || !lin_rank || !out_words) return fail(GF2BV_ERR_ARG, "null pointer");
	if (max_enum < 0 || max_enum > D::kMaxEnum) return fail(GF2BV_ERR_ARG, "max_enum must be 0..40");
	if (max_solutions < 0) return fail(GF2BV_ERR_ARG, "max_solutions must be >= 0");
	return search_alloc(D::times(), dimension, words, max_solutions, device, count, lin_rank, out_words,
	                    [&](hipStream_t st, std::vector<u64> &pts, std::vector<u64> &coef, u64 *total, bool *gave_up) {
		return D::collect(origin, basis, dimension, words, n_lin, max_enum, device, st, pts, coef, total, reinterpret_cast<i64 *>(lin_rank),
		                  gave_up);
	});
}

// gf2bv_*_search: the points of `alloc` (gf2bv_*_search_alloc) copied into the caller's buffer
template <class Alloc>
int search_space_copy(Alloc alloc, int64_t words, int64_t max_solutions, int64_t *count, uint64_t *out_words_)
{
	if (max_solutions > 0 && !out_words_) return fail(GF2BV_ERR_ARG, "null pointer");
	uint64_t *pts = nullptr;
	const int rc = alloc(&pts);
	if (rc == GF2BV_OK && pts) memcpy(out_words_, pts, sizeof(uint64_t) * (size_t)(std::min<int64_t>(*count, max_solutions) * words));
	gf2bv_quad_free(pts);
	return rc;
}

void search_last_times(const QuadTimes &t, double *out8)
{
	if (!out8) return;
	const double v[8] = {t.reduce, t.forms, t.affine, t.search, t.relin, t.total, (double)t.levels, (double)t.candidates};
	std::copy(v, v + 8, out8);
}

}  // namespace

extern "C" {

int gf2bv_quad_plan(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                    int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms_, int64_t forms_cap)
{
	return catching([&] { return search_plan<QuadDegree>(origin_, basis_, dimension, words, n_lin, false, -1, r, r_eff, m, form_words, forms_, forms_cap); });
}
int gf2bv_quad_plan_device(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin, int device,
                           int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms_, int64_t forms_cap)
{
	return guarded([&] { return search_plan<QuadDegree>(origin_, basis_, dimension, words, n_lin, true, device, r, r_eff, m, form_words, forms_, forms_cap); });
}
int gf2bv_quad_points(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                      const uint64_t *ys_, int64_t nys, int64_t y_words, uint64_t *out_words_)
{
	return catching([&] { return search_points<QuadDegree>(origin_, basis_, dimension, words, n_lin, ys_, nys, y_words, out_words_); });
}
int gf2bv_quad_forms_search(const uint64_t *forms_, int64_t m, int64_t r_eff, int device, int64_t max_out, int64_t *count,
                            uint64_t *out_)
{
	return guarded([&] { return search_forms<QuadDegree>(forms_, m, r_eff, device, max_out, count, out_); });
}
int gf2bv_quad_search(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                      int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t *out_words_)
{
	return search_space_copy([&](uint64_t **pts) {
		return gf2bv_quad_search_alloc(origin_, basis_, dimension, words, n_lin, max_enum, max_solutions, device, count, lin_rank, pts);
	}, words, max_solutions, count, out_words_);
}
int gf2bv_quad_search_alloc(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                            int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t **out_words)
{
	return guarded([&] {
		return search_space_alloc<QuadDegree>(origin_, basis_, dimension, words, n_lin, max_enum, max_solutions, device, count, lin_rank, out_words);
	});
}
void gf2bv_quad_last_times(double *out8) { search_last_times(QuadDegree::times(), out8); }

int gf2bv_cubic_plan(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                    int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms_, int64_t forms_cap)
{
	return catching([&] { return search_plan<CubicDegree>(origin_, basis_, dimension, words, n_lin, false, -1, r, r_eff, m, form_words, forms_, forms_cap); });
}
int gf2bv_cubic_plan_device(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin, int device,
                           int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms_, int64_t forms_cap)
{
	return guarded([&] { return search_plan<CubicDegree>(origin_, basis_, dimension, words, n_lin, true, device, r, r_eff, m, form_words, forms_, forms_cap); });
}
int gf2bv_cubic_points(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                      const uint64_t *ys_, int64_t nys, int64_t y_words, uint64_t *out_words_)
{
	return catching([&] { return search_points<CubicDegree>(origin_, basis_, dimension, words, n_lin, ys_, nys, y_words, out_words_); });
}
int gf2bv_cubic_forms_search(const uint64_t *forms_, int64_t m, int64_t r_eff, int device, int64_t max_out, int64_t *count,
                            uint64_t *out_)
{
	return guarded([&] { return search_forms<CubicDegree>(forms_, m, r_eff, device, max_out, count, out_); });
}
int gf2bv_cubic_search(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                      int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t *out_words_)
{
	return search_space_copy([&](uint64_t **pts) {
		return gf2bv_cubic_search_alloc(origin_, basis_, dimension, words, n_lin, max_enum, max_solutions, device, count, lin_rank, pts);
	}, words, max_solutions, count, out_words_);
}
int gf2bv_cubic_search_alloc(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                            int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t **out_words)
{
	return guarded([&] {
		return search_space_alloc<CubicDegree>(origin_, basis_, dimension, words, n_lin, max_enum, max_solutions, device, count, lin_rank, out_words);
	});
}
void gf2bv_cubic_last_times(double *out8) { search_last_times(CubicDegree::times(), out8); }

int gf2bv_quartic_plan(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                    int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms_, int64_t forms_cap)
{
	return catching([&] { return search_plan<QuarticDegree>(origin_, basis_, dimension, words, n_lin, false, -1, r, r_eff, m, form_words, forms_, forms_cap); });
}
int gf2bv_quartic_plan_device(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin, int device,
                           int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms_, int64_t forms_cap)
{
	return guarded([&] { return search_plan<QuarticDegree>(origin_, basis_, dimension, words, n_lin, true, device, r, r_eff, m, form_words, forms_, forms_cap); });
}
int gf2bv_quartic_points(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                      const uint64_t *ys_, int64_t nys, int64_t y_words, uint64_t *out_words_)
{
	return catching([&] { return search_points<QuarticDegree>(origin_, basis_, dimension, words, n_lin, ys_, nys, y_words, out_words_); });
}
int gf2bv_quartic_forms_search(const uint64_t *forms_, int64_t m, int64_t r_eff, int device, int64_t max_out, int64_t *count,
                            uint64_t *out_)
{
	return guarded([&] { return search_forms<QuarticDegree>(forms_, m, r_eff, device, max_out, count, out_); });
}
int gf2bv_quartic_search(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                      int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t *out_words_)
{
	return search_space_copy([&](uint64_t **pts) {
		return gf2bv_quartic_search_alloc(origin_, basis_, dimension, words, n_lin, max_enum, max_solutions, device, count, lin_rank, pts);
	}, words, max_solutions, count, out_words_);
}
int gf2bv_quartic_search_alloc(const uint64_t *origin_, const uint64_t *basis_, int64_t dimension, int64_t words, int64_t n_lin,
                            int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t **out_words)
{
	return guarded([&] {
		return search_space_alloc<QuarticDegree>(origin_, basis_, dimension, words, n_lin, max_enum, max_solutions, device, count, lin_rank, out_words);
	});
}
void gf2bv_quartic_last_times(double *out8) { search_last_times(QuarticDegree::times(), out8); }

void gf2bv_quad_free(uint64_t *words) { free(words); }

}  // extern "C"

// =================================================================================================
// Expansion of factored equations: a linear form plus products of two (degree 3: and of three, degree 4: and of four) forms become the
// linearised rows of the C-ABI layout on the device (k_quad_expand, k_cubic_expand, k_quartic_expand), where gf2bv_solve_device and
// the factor entries read them.
namespace {

constexpr i64 kExpandLdsBytes = 65536;                 // what every expansion kernel below may take of a workgroup's LDS ...
constexpr i64 kQuarticLdsBytes = 160 * 1024 - 256;     // ... but k_quartic_expand, which stages cubic rows there (the attribute is raised above 64 KiB)

// the workgroup of every expansion kernel: a thread per two words of an output row
unsigned expand_block(i64 stride) { return (unsigned)std::min<i64>(256, round_up(std::max<i64>(stride / 2, 1), 64)); }

// The factored form, in host or in device memory: a linear form a row plus, per group, products of `arity` forms -- rows off[r] ..
// off[r + 1] of each of the group's operand arrays.  One group (degree 2): the products follow QuadraticSystem._mul_bit, over
// n + C(n,2) columns; two and three groups (degree 3, 4): affine forms and products exact in GF(2)[x] / (x_i^2 + x_i), over the
// columns of degree-3 and of degree-4 XL
struct TermGroup {
	int arity;                         // 2, 3, 4 in this order
	const i64 *off;                    // rows_live + 1
	const u64 *ops[4];                 // the first `arity`
	bool lacks_operand() const { return std::any_of(ops, ops + arity, [](const u64 *p) { return !p; }); }
};
struct Terms {
	const u64 *lin;                    // rows_live x wl
	i64 rows_live, rows, n;
	int ngroups = 0;
	TermGroup group[3] = {};
	// every group as { off, operand, operand, ... }, in the order of the exported entries' argument lists
	Terms(const void *lin, i64 rows_live, i64 rows, i64 n_lin, std::initializer_list<std::initializer_list<const void *>> groups)
		: lin((const u64 *)lin), rows_live(rows_live), rows(rows), n(n_lin)
	{
		for (const auto &g : groups) {
			TermGroup &t = group[ngroups];
			t.arity = 2 + ngroups++;
			t.off = (const i64 *)*g.begin();
			std::transform(g.begin() + 1, g.end(), t.ops, [](const void *p) { return (const u64 *)p; });
		}
	}
	int degree() const { return ngroups + 1; }
	i64 wl() const { return (n + 1 + 63) / 64; }
	i64 cols3() const { return n + n * (n - 1) / 2 + n * (n - 1) * (n - 2) / 6; }
	i64 cols() const
	{
		if (ngroups == 3) return n > 1024 ? (1ll << 40) : cols3() + n * (n - 1) * (n - 2) / 6 * (n - 3) / 4;      // (C(1025,4) is far above any row)
		return ngroups == 2 ? cols3() : n + n * (n - 1) / 2;
	}
	i64 wt() const { return (cols() + 1 + 63) / 64; }
};

// What the expansion kernel of a degree is launched with: tch[g] terms of group g of a row in LDS at a time
struct ExpandLaunch { int tch[3]; unsigned block; size_t lds; };
ExpandLaunch expand_launch(int degree, i64 n, i64 stride)
{
	const i64 wl = (n + 1 + 63) / 64;
	auto chunk = [](i64 most, i64 fit) { return (int)std::max<i64>(1, std::min(most, fit)); };
	if (degree == 2) {                 // k_quad_expand and its batched form
		const int tch = chunk(8, (kExpandLdsBytes / 8 / wl - 1) / 2);
		return { { tch, 0, 0 }, expand_block(stride), sizeof(u64) * (size_t)((1 + 2 * tch) * wl) };
	}
	if (degree == 3) {                 // k_cubic_expand: the cubic operands served first where a form is long
		const i64 avail = kExpandLdsBytes / 8 / wl - 1;            // operands beside the linear part
		const int tch3 = chunk(8, avail / 5), tch2 = chunk(8, (avail - 3 * tch3) / 2);
		return { { tch2, tch3, 0 }, expand_block(stride), sizeof(u64) * (size_t)((1 + 2 * tch2 + 3 * tch3) * wl) };
	}
	// k_quartic_expand: beside the linear part and the terms, 1 + tch4 staged cubic rows of w3 words.  The staged rows come first:
	// with every chunk at 1 a pass needs 10 wl + 2 w3 words, which is what bounds n_lin (about 157); lds above kQuarticLdsBytes:
	// this n_lin does not fit
	const i64 w3 = n > 1024 ? (1ll << 30) : (n + n * (n - 1) / 2 + n * (n - 1) * (n - 2) / 6 + 1 + 63) / 64;
	i64 rest = kQuarticLdsBytes / 8 - wl - w3;
	const int tch4 = chunk(4, rest / 3 / (4 * wl + w3));
	rest -= tch4 * (4 * wl + w3);
	const int tch3 = chunk(8, rest / 2 / (3 * wl));
	rest -= tch3 * 3 * wl;
	const int tch2 = chunk(8, rest / (2 * wl));
	return { { tch2, tch3, tch4 }, expand_block(stride), sizeof(u64) * (size_t)((1 + 2 * tch2 + 3 * tch3 + 4 * tch4) * wl + (1 + tch4) * w3) };
}

// The shape of a factored system; `host`: the offsets can be read (each array starts at 0 and never decreases; operands wherever
// they say there are terms)
int check_terms(const Terms &t, bool host)
{
	static const char *const kColsText[3] = { "n_lin must be at least 1 and n_lin + n_lin(n_lin-1)/2 below 2^31 - 64",
	                                          "n_lin must be at least 1 and n_lin + C(n_lin,2) + C(n_lin,3) below 2^31 - 64",
	                                          "n_lin must be at least 1 and n_lin + C(n_lin,2) + C(n_lin,3) + C(n_lin,4) below 2^31 - 64" };
	auto any_group = [&](auto &&pred) { return std::any_of(t.group, t.group + t.ngroups, pred); };
	if (!t.lin && t.rows_live > 0) return fail(GF2BV_ERR_ARG, "null pointer");
	if (any_group([](const TermGroup &g) { return !g.off; })) return fail(GF2BV_ERR_ARG, "null pointer");
	if (t.n < 1 || t.n > 65535 || t.cols() >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, kColsText[t.ngroups - 1]);
	if (t.rows < 0 || t.rows >= (1ll << 31) - 64 || t.rows_live < 0 || t.rows_live > t.rows)
		return fail(GF2BV_ERR_ARG, "rows_live must be 0..rows");
	if (t.degree() == 4 && (i64)expand_launch(4, t.n, 2).lds > kQuarticLdsBytes)
		return fail(GF2BV_ERR_ARG, "the operands and the staged cubic rows of this n_lin do not fit the expansion kernel's LDS (160 KiB)");
	if (t.degree() == 3 && (i64)expand_launch(3, t.n, 2).lds > kExpandLdsBytes)
		return fail(GF2BV_ERR_ARG, "the operands of this n_lin do not fit the expansion kernel's LDS (64 KiB)");
	if (!host) {
		if (!t.lin || any_group([](const TermGroup &g) { return g.lacks_operand(); })) return fail(GF2BV_ERR_ARG, "null pointer");
		return GF2BV_OK;
	}
	if (any_group([](const TermGroup &g) { return g.off[0] != 0; })) return fail(GF2BV_ERR_ARG, "term offsets must start at 0");
	for (i64 r = 0; r < t.rows_live; r++)
		if (any_group([r](const TermGroup &g) { return g.off[r + 1] < g.off[r]; })) return fail(GF2BV_ERR_ARG, "term offsets must not decrease");
	if (any_group([&](const TermGroup &g) { return g.lacks_operand() && g.off[t.rows_live] > 0; })) return fail(GF2BV_ERR_ARG, "null pointer");
	return GF2BV_OK;
}

// (device pointers, already checked) the kernel on `st`
int enqueue_quad_expand(const Terms &q, u64 *d_aug, i64 stride, hipStream_t st)
{
	if (q.rows == 0) return GF2BV_OK;
	const ExpandLaunch l = expand_launch(2, q.n, stride);
	const TermGroup &g = q.group[0];
	const unsigned grid = (unsigned)std::min<i64>(q.rows, 256 * 8);
	hipLaunchKernelGGL(k_quad_expand, dim3(grid), dim3(l.block), l.lds, st, q.lin, g.off, g.ops[0], g.ops[1], q.rows_live, q.rows, (int)q.n,
	                   (int)q.wl(), l.tch[0], d_aug, stride);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// The batched form: nsys (not negative) systems over one concatenated term set, system s owning the rows sys_off[s] .. sys_off[s + 1],
// at most q.rows of them; q.rows_live becomes sys_off[nsys], the rows of the whole set.  Quadratic terms only: there is no batched cubic kernel
int check_quad_batch(Terms &q, const i64 *sys_off, i64 nsys)
{
	if (!sys_off) return fail(GF2BV_ERR_ARG, "null pointer");
	if (q.rows < 0 || q.rows >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, "rows must be 0 .. 2^31 - 65");
	if (sys_off[0] != 0) return fail(GF2BV_ERR_ARG, "system row offsets must start at 0");
	for (i64 s = 0; s < nsys; s++) {
		if (sys_off[s + 1] < sys_off[s]) return fail(GF2BV_ERR_ARG, "system row offsets must not decrease");
		if (sys_off[s + 1] - sys_off[s] > q.rows) return fail(GF2BV_ERR_ARG, "a system's live rows must be 0..rows");
	}
	if (sys_off[nsys] >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, "the rows of all systems together must stay below 2^31 - 64");
	const i64 rows = q.rows;
	q.rows_live = q.rows = sys_off[nsys];          // (check_terms: the concatenated set as one system of all its rows)
	const int rc = check_terms(q, true);
	q.rows = rows;
	return rc;
}

// (device pointers, already checked) the batched kernel on `st`: system s at d_aug + s x sys_stride, q.rows x stride words
int enqueue_quad_expand_batch(const Terms &q, const i64 *d_sys_off, i64 nsys, u64 *d_aug, i64 stride, i64 sys_stride, hipStream_t st)
{
	if (q.rows == 0 || nsys == 0) return GF2BV_OK;
	const ExpandLaunch l = expand_launch(2, q.n, stride);
	const TermGroup &g = q.group[0];
	// a workgroup per row at a time; a few thousand workgroups in all, however many systems share the launch
	const unsigned gx = (unsigned)std::min<i64>(q.rows, std::max<i64>(256, 256 * 8 / nsys));
	for (i64 s0 = 0; s0 < nsys; s0 += 65535) {      // (grid y holds 65535 systems)
		const unsigned ns = (unsigned)std::min<i64>(65535, nsys - s0);
		hipLaunchKernelGGL(k_quad_expand_batch, dim3(gx, ns), dim3(l.block), l.lds, st, q.lin, g.off, g.ops[0], g.ops[1], d_sys_off + s0, q.rows,
		                   (int)q.n, (int)q.wl(), l.tch[0], d_aug + s0 * sys_stride, stride, sys_stride);
	}
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// (device pointers, already checked) the kernel on `st`
int enqueue_cubic_expand(const Terms &c, u64 *d_aug, i64 stride, hipStream_t st)
{
	if (c.rows == 0) return GF2BV_OK;
	const ExpandLaunch l = expand_launch(3, c.n, stride);
	const TermGroup &q = c.group[0], &u = c.group[1];
	const unsigned grid = (unsigned)std::min<i64>(c.rows, 256 * 16);
	hipLaunchKernelGGL(k_cubic_expand, dim3(grid), dim3(l.block), l.lds, st, c.lin, q.off, q.ops[0], q.ops[1], u.off, u.ops[0], u.ops[1], u.ops[2],
	                   c.rows_live, c.rows, (int)c.n, (int)c.wl(), l.tch[0], l.tch[1], d_aug, stride);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// (device pointers, already checked; the device is current) the kernel on `st`
int enqueue_quartic_expand(const Terms &c, u64 *d_aug, i64 stride, hipStream_t st)
{
	if (c.rows == 0) return GF2BV_OK;
	const ExpandLaunch l = expand_launch(4, c.n, stride);
	const TermGroup &q = c.group[0], &u = c.group[1], &v = c.group[2];
	if ((i64)l.lds > kExpandLdsBytes) {                // (a function attribute holds per device: raised once on each that needs it)
		static std::mutex mu;
		static std::map<int, bool> raised;
		int device = 0;
		HIPCHK(hipGetDevice(&device));
		std::lock_guard<std::mutex> lk(mu);
		if (!raised[device]) {
			HIPCHK(hipFuncSetAttribute((const void *)k_quartic_expand, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQuarticLdsBytes));
			raised[device] = true;
		}
	}
	const unsigned grid = (unsigned)std::min<i64>(c.rows, 256 * 16);
	hipLaunchKernelGGL(k_quartic_expand, dim3(grid), dim3(l.block), l.lds, st, c.lin, q.off, q.ops[0], q.ops[1], u.off, u.ops[0], u.ops[1], u.ops[2],
	                   v.off, v.ops[0], v.ops[1], v.ops[2], v.ops[3], c.rows_live, c.rows, (int)c.n, (int)c.wl(), (int)((c.cols3() + 1 + 63) / 64),
	                   l.tch[0], l.tch[1], l.tch[2], d_aug, stride);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// (device pointers, already checked) the kernel of the terms' degree on `st`
int enqueue_expand(const Terms &t, u64 *d_aug, i64 stride, hipStream_t st)
{
	if (t.degree() == 4) return enqueue_quartic_expand(t, d_aug, stride, st);
	return t.degree() == 3 ? enqueue_cubic_expand(t, d_aug, stride, st) : enqueue_quad_expand(t, d_aug, stride, st);
}

// XL (k_xl3_expand, k_xl4_expand): m quadratic rows over n unknowns -- the rows k_quad_expand writes -- become `rows` rows over the
// monomials of degree <= `degree`: each equation, its product with every unknown and (degree 4) with every pair of unknowns, then zeros.
// src = 3 (k_xl4_cubic_expand, degree 4 only): the m rows are cubic -- the rows k_cubic_expand writes -- and the multipliers stop at
// the unknowns
struct XlShape {
	int degree;
	int src;                           // the degree of the source rows
	i64 m, n, rows;
	XlShape(int degree, int src, i64 m, i64 n, i64 rows = 0) : degree(degree), src(src), m(m), n(n), rows(rows) {}
	i64 cols2() const { return n + n * (n - 1) / 2; }
	i64 cols3() const { return cols2() + n * (n - 1) * (n - 2) / 6; }
	i64 cols4() const { return cols3() + n * (n - 1) * (n - 2) * (n - 3) / 24; }
	i64 cols() const { return degree == 4 ? cols4() : cols3(); }
	i64 per_eq() const { return degree == 4 && src == 2 ? 1 + cols2() : n + 1; }      // rows an equation owns
	i64 w2() const { return (cols2() + 1 + 63) / 64; }         // words of a quadratic row
	i64 wsrc() const { return src == 3 ? (cols3() + 1 + 63) / 64 : w2(); }      // words of a source row, which the kernel holds in LDS
	i64 wt() const { return (cols() + 1 + 63) / 64; }
	i64 live() const { return m * per_eq(); }
};

// The shape, and the source stride against it; no pointer is looked at.  `pad`: a solve entry, whose rows are the live ones padded up
// to the columns
int check_xl(XlShape &x, i64 quad_stride, bool pad = false)
{
	const bool d4 = x.degree == 4 && x.src == 2, cubic = x.src == 3;
	if (cubic && x.degree != 4) return fail(GF2BV_ERR_ARG, "cubic rows take degree 4");
	if (x.n < 1 || x.n > 65535 || x.cols() >= (1ll << 31) - 64)
		return fail(GF2BV_ERR_ARG, d4 || cubic ? "n_lin must be at least 1 and n_lin + C(n_lin,2) + C(n_lin,3) + C(n_lin,4) below 2^31 - 64"
		                                       : "n_lin must be at least 1 and n_lin + C(n_lin,2) + C(n_lin,3) below 2^31 - 64");
	if (x.m < 0 || x.m >= (1ll << 31) - 64 || x.live() >= (1ll << 31) - 64)
		return fail(GF2BV_ERR_ARG, d4 ? "m(1 + n_lin + C(n_lin,2)) must stay below 2^31 - 64" : "m(n_lin + 1) must stay below 2^31 - 64");
	if (pad) x.rows = std::max(x.live(), x.cols());
	if (x.rows >= (1ll << 31) - 64 || x.rows < x.live())
		return fail(GF2BV_ERR_ARG, d4 ? "rows must be at least m(1 + n_lin + C(n_lin,2)) and below 2^31 - 64"
		                              : "rows must be at least m(n_lin + 1) and below 2^31 - 64");
	if (x.wsrc() * 8 > kExpandLdsBytes)
		return fail(GF2BV_ERR_ARG, cubic ? "a cubic row of this n_lin does not fit the expansion kernel's LDS (64 KiB)"
		                                 : "a quadratic row of this n_lin does not fit the expansion kernel's LDS (64 KiB)");
	if (quad_stride < x.wsrc())
		return fail(GF2BV_ERR_ARG, cubic ? "cubic_stride_words does not cover the cubic columns and the constant"
		                                 : "quad_stride_words does not cover the quadratic columns and the constant");
	return GF2BV_OK;
}

// Degree 4: the workgroups of one system take (equation, part) units -- every parts-th row of an equation's rows -- a few thousand
// units over all `nsys` systems where the equations allow it
int xl4_parts(const XlShape &x, i64 nsys)
{
	return (int)std::max<i64>(1, std::min<i64>(x.per_eq(), 4096 / std::max<i64>(x.m * nsys, 1)));
}

// (device pointers, already checked) the kernel on `st`.  Degree 3: a few thousand workgroups, each a contiguous span of the rows;
// degree 4: a workgroup per (equation, part) unit; cubic rows: degree 3's spans
int enqueue_xl_expand(const XlShape &x, const u64 *d_quad, i64 quad_stride, u64 *d_aug, i64 stride, hipStream_t st)
{
	if (x.rows == 0) return GF2BV_OK;
	const unsigned block = expand_block(stride);
	if (x.src == 3) {
		const unsigned grid = (unsigned)std::min<i64>(x.rows, 256 * 16);
		hipLaunchKernelGGL(k_xl4_cubic_expand, dim3(grid), dim3(block), sizeof(u64) * (size_t)x.wsrc(), st, d_quad, x.m, quad_stride, (int)x.n,
		                   (int)x.wsrc(), x.rows, d_aug, stride);
	} else if (x.degree == 4) {
		const int parts = xl4_parts(x, 1);
		const unsigned grid = (unsigned)std::min<i64>(std::max<i64>(x.m * parts, std::min<i64>(x.rows - x.live(), 4096)), 1 << 20);
		hipLaunchKernelGGL(k_xl4_expand, dim3(grid), dim3(block), sizeof(u64) * (size_t)x.w2(), st, d_quad, x.m, quad_stride, (int)x.n,
		                   (int)x.w2(), x.rows, parts, d_aug, stride);
	} else {
		const unsigned grid = (unsigned)std::min<i64>(x.rows, 256 * 16);
		hipLaunchKernelGGL(k_xl3_expand, dim3(grid), dim3(block), sizeof(u64) * (size_t)x.w2(), st, d_quad, x.m, quad_stride, (int)x.n,
		                   (int)x.w2(), x.rows, d_aug, stride);
	}
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// (device pointers, already checked) the batched kernel on `st`: system s reads its x.m rows at d_quad + s x quad_sys_stride and writes
// x.rows rows at d_aug + s x sys_stride
int enqueue_xl_expand_batch(const XlShape &x, const u64 *d_quad, i64 quad_sys_stride, i64 quad_stride, i64 nsys, u64 *d_aug, i64 stride,
                            i64 sys_stride, hipStream_t st)
{
	if (x.rows == 0 || nsys == 0) return GF2BV_OK;
	const unsigned block = expand_block(stride);
	// degree 3 and cubic rows: contiguous spans of rows per workgroup, a few thousand workgroups in all where the systems are many
	const int parts = xl4_parts(x, nsys);
	const bool units = x.degree == 4 && x.src == 2;
	const unsigned gx = units ? (unsigned)std::min<i64>(std::max<i64>(x.m * parts, std::min<i64>(x.rows - x.live(), 256)), 1 << 20)
	                          : (unsigned)std::min<i64>(x.rows, std::max<i64>(256, 256 * 16 / nsys));
	for (i64 s0 = 0; s0 < nsys; s0 += 65535) {         // (grid y holds 65535 systems)
		const unsigned ns = (unsigned)std::min<i64>(65535, nsys - s0);
		if (x.src == 3)
			hipLaunchKernelGGL(k_xl4_cubic_expand_batch, dim3(gx, ns), dim3(block), sizeof(u64) * (size_t)x.wsrc(), st, d_quad + s0 * quad_sys_stride,
			                   quad_sys_stride, x.m, quad_stride, (int)x.n, (int)x.wsrc(), x.rows, d_aug + s0 * sys_stride, stride, sys_stride);
		else if (x.degree == 4)
			hipLaunchKernelGGL(k_xl4_expand_batch, dim3(gx, ns), dim3(block), sizeof(u64) * (size_t)x.w2(), st, d_quad + s0 * quad_sys_stride,
			                   quad_sys_stride, x.m, quad_stride, (int)x.n, (int)x.w2(), x.rows, parts, d_aug + s0 * sys_stride, stride, sys_stride);
		else
			hipLaunchKernelGGL(k_xl3_expand_batch, dim3(gx, ns), dim3(block), sizeof(u64) * (size_t)x.w2(), st, d_quad + s0 * quad_sys_stride,
			                   quad_sys_stride, x.m, quad_stride, (int)x.n, (int)x.w2(), x.rows, d_aug + s0 * sys_stride, stride, sys_stride);
	}
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// Hybrid XL (k_quad_specialise, k_cubic_specialise): f guessed unknowns substituted into m rows of degree `src` over n unknowns, for
// the assignments a0 .. a0 + na - 1; every assignment leaves the system `x` of m rows of that degree over n - f unknowns
struct GuessShape {
	i64 m, n, f, a0, na;
	int src;                           // the degree of the source rows
	SpecGuess g{};
	XlShape x;                         // (check_guess fills m and n; the degree matters to the solve entries only)
	GuessShape(i64 m, i64 n_lin, i64 nguess, i64 a0, i64 na, int degree = 3, int src = 2)
		: m(m), n(n_lin), f(nguess), a0(a0), na(na), src(src), x(degree, src, 0, 0) {}
	i64 cols() const { return n + n * (n - 1) / 2 + (src == 3 ? n * (n - 1) * (n - 2) / 6 : 0); }      // the source's columns
	i64 wsrc() const { return (cols() + 1 + 63) / 64; }                // words of a source row
	i64 lds_bytes() const                                              // what the source's kernel holds (see there)
	{
		const i64 wv = (x.n + 63) / 64;
		if (src == 3) return 8 * (wsrc() + x.wsrc() + f * ((x.cols2() + 63) / 64) + f * (f - 1) / 2 * (wv + 1) + 1 + f) + 4 * x.n;
		return 8 * (wsrc() + x.w2() + f * (wv + 2)) + 4 * x.n;
	}
};

// The guess, the range of assignments and the source stride; no device pointer is looked at
int check_guess(GuessShape &s, const int32_t *guess, i64 quad_stride)
{
	const bool cubic = s.src == 3;
	if (s.n < 1 || s.n > 65535 || s.cols() >= (1ll << 31) - 64)
		return fail(GF2BV_ERR_ARG, cubic ? "n_lin must be at least 1 and n_lin + C(n_lin,2) + C(n_lin,3) below 2^31 - 64"
		                                 : "n_lin must be at least 1 and n_lin + C(n_lin,2) below 2^31 - 64");
	if (s.f < 0 || s.f > std::min<i64>(s.n - 1, 30)) return fail(GF2BV_ERR_ARG, "nguess must be 0 .. min(n_lin - 1, 30)");
	if (!guess && s.f > 0) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 t = 0; t < s.f; t++) {
		if (guess[t] < 0 || guess[t] >= s.n) return fail(GF2BV_ERR_ARG, "a guessed unknown must be 0 .. n_lin - 1");
		for (i64 u = 0; u < t; u++)
			if (guess[u] == guess[t]) return fail(GF2BV_ERR_ARG, "a guessed unknown is repeated");
		s.g.g[t] = guess[t];
	}
	if (s.a0 < 0 || s.na < 0 || s.a0 > (1ll << s.f) || s.na > (1ll << s.f) - s.a0)
		return fail(GF2BV_ERR_ARG, "the assignments a0 .. a0 + na - 1 must lie in 0 .. 2^nguess - 1");
	if (s.m < 0 || s.m >= (1ll << 31) - 64 || s.na * std::max<i64>(s.m, 1) >= (1ll << 31) - 64)
		return fail(GF2BV_ERR_ARG, "m and na x m must stay below 2^31 - 64");
	s.x.m = s.m; s.x.n = s.n - s.f;
	if (quad_stride < s.wsrc())
		return fail(GF2BV_ERR_ARG, cubic ? "cubic_stride_words does not cover the cubic columns and the constant"
		                                 : "quad_stride_words does not cover the quadratic columns and the constant");
	if (s.lds_bytes() > kExpandLdsBytes)
		return fail(GF2BV_ERR_ARG, cubic ? "the cubic row, its specialised form and the guess vectors do not fit the specialisation kernel's LDS (64 KiB)"
		                                 : "the quadratic row, its specialised form and the guess vectors do not fit the specialisation kernel's LDS (64 KiB)");
	return GF2BV_OK;
}

// The systems behind a solve entry: each assignment's expansion padded up to its columns, all of them one batch
int check_guess_solve(GuessShape &s, int mode)
{
	int rc = check_xl(s.x, s.x.wsrc(), true);
	if (rc) return rc;
	if (s.na * s.x.rows >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, "the rows of all assignments' systems together must stay below 2^31 - 64");
	return check_shape(s.x.rows, s.x.cols(), mode);
}

// (device pointers, already checked) the source's kernel on `st`: system a - a0 at d_out + (a - a0) x sys_stride, m rows out_stride
// words apart
int enqueue_specialise(const GuessShape &s, const u64 *d_quad, i64 quad_stride, u64 *d_out, i64 out_stride, i64 sys_stride, hipStream_t st)
{
	if (s.m == 0 || s.na == 0) return GF2BV_OK;
	const unsigned gx = (unsigned)std::min<i64>(s.m, 1024);
	const unsigned gy = (unsigned)std::max<i64>(1, std::min<i64>({ s.na, 65535, 2048 / gx }));      // a couple of thousand workgroups
	const int vec = !(out_stride & 1) && !(sys_stride & 1) && !((uintptr_t)d_out & 15);
	hipLaunchKernelGGL(s.src == 3 ? k_cubic_specialise : k_quad_specialise, dim3(gx, gy), dim3(256), (size_t)s.lds_bytes(), st, d_quad, s.m,
	                   quad_stride, (int)s.n, (int)s.wsrc(), s.g, (int)s.f, s.a0, s.na, d_out, out_stride, sys_stride, vec);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// What one assignment's system holds on the device while a solve entry runs: its specialised rows and its padded expansion
i64 guess_system_bytes(const XlShape &x) { return 8 * (x.m * round_up(x.wsrc(), 2) + x.rows * round_up(x.wt(), 2)); }

// A factored system of host memory (checked) staged on the device for the length of an entry: the terms uploaded and expanded into
// d_aug (q.rows x ds words a system) on ONE pool stream, where the entry underneath is ordered behind the expansion.  Stream and
// buffers go back by the holder's rule: a handle has its own copy by then, a result is on the host.
struct QuadStage {
	Held held;
	const bool nomem;                  // a refused pool buffer is GF2BV_ERR_NOMEM (the expanded rows of a large system or batch may not fit; an
	                                   // append tells a refusal, which leaves the handle as it was, from a failure that does not); the two
	                                   // first entries, gf2bv_quad_expand_words and gf2bv_solve_quad_terms, keep their GF2BV_ERR_HIP
	u64 *d_aug = nullptr, *d_rhs = nullptr;
	i64 ds = 0;
	u64 *d_xl = nullptr;               // the XL expansion of the rows in d_aug (expand_xl), xs words a row: both are held at once
	i64 xs = 0;
	u64 *d_spec = nullptr;             // hybrid XL: the rows in d_aug specialised for na assignments (specialise), ss words a row, m x ss a system
	i64 ss = 0;
	explicit QuadStage(int device, bool nomem = true) : held(device), nomem(nomem) {}

	int open()                         // the stream, once
	{
		if (!held.st) HIPCHK(held.stream(0));
		return GF2BV_OK;
	}

	int alloc(void **out, size_t bytes)
	{
		if (nomem) return held.alloc(out, bytes, "the factored rows or their expansion do not fit on the device", "expansion buffers");
		const hipError_t e = held.get(out, bytes);
		return e == hipSuccess ? GF2BV_OK : fail(GF2BV_ERR_HIP, "expansion buffers", e);
	}
	template <class T>
	int upload(T **d, const T *h, size_t bytes)
	{
		if (int rc = alloc((void **)d, bytes)) return rc;
		if (bytes) HIPCHK(hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, held.st));
		return GF2BV_OK;
	}
	// Upload of the term groups and expansion (the kernel of t.degree()), with rows `stride` words apart rounded up to an even `ds`; sys_off:
	// the batched form, nsys systems (t as check_quad_batch left it); rhs: right-hand sides that go up into d_rhs in front of the expansion
	int expand(Terms t, i64 stride, const i64 *sys_off = nullptr, i64 nsys = 1, const u64 *rhs = nullptr, size_t rhs_bytes = 0)
	{
		if (sys_off && t.degree() != 2) return fail(GF2BV_ERR_ARG, "the batched expansion takes quadratic terms");
		if (int rc = open()) return rc;
		const i64 wl = t.wl();
		i64 *d_sys = nullptr;
		int rc = upload((u64 **)&t.lin, t.lin, sizeof(u64) * (size_t)(t.rows_live * wl));
		// a group's offsets, then its operands: each host pointer of `t` becomes the device copy
		for (TermGroup *g = t.group; g < t.group + t.ngroups; g++) {
			const size_t bytes = sizeof(u64) * (size_t)(g->off[t.rows_live] * wl);
			if (!rc) rc = upload((i64 **)&g->off, g->off, sizeof(i64) * (size_t)(t.rows_live + 1));
			for (int k = 0; k < g->arity; k++)
				if (!rc) rc = upload((u64 **)&g->ops[k], g->ops[k], bytes);
		}
		if (!rc && sys_off) rc = upload(&d_sys, sys_off, sizeof(i64) * (size_t)(nsys + 1));
		ds = round_up(stride, 2);
		if (!rc) rc = alloc((void **)&d_aug, sizeof(u64) * (size_t)(nsys * t.rows * ds));
		if (!rc && rhs) rc = upload(&d_rhs, rhs, rhs_bytes);
		if (rc) return rc;
		if (sys_off) return enqueue_quad_expand_batch(t, d_sys, nsys, d_aug, ds, t.rows * ds, held.st);
		return enqueue_expand(t, d_aug, ds, held.st);
	}
	// Quadratic rows that are expanded already (host memory, `stride` words apart) into d_aug as they are
	int upload_rows(const u64 *quad, i64 m, i64 stride)
	{
		if (int rc = open()) return rc;
		ds = stride;
		return upload(&d_aug, quad, sizeof(u64) * (size_t)(m * stride));
	}
	// The XL expansion (x.degree, x.src) of the x.m quadratic or cubic rows in d_aug into d_xl, x.rows rows `stride` words apart rounded up to an even xs,
	// behind whatever wrote d_aug on the stream
	int expand_xl(const XlShape &x, i64 stride)
	{
		xs = round_up(stride, 2);
		if (int rc = alloc((void **)&d_xl, sizeof(u64) * (size_t)(x.rows * xs))) return rc;
		return enqueue_xl_expand(x, d_aug, ds, d_xl, xs, held.st);
	}
	// The rows in d_aug specialised for every assignment of `g` into d_spec, rows `stride` words apart
	int specialise(const GuessShape &g, i64 stride)
	{
		ss = stride;
		if (int rc = alloc((void **)&d_spec, sizeof(u64) * (size_t)(g.na * g.m * ss))) return rc;
		return enqueue_specialise(g, d_aug, ds, d_spec, ss, g.m * ss, held.st);
	}
	// The XL expansions (x.degree, x.src) of nsys systems of x.m quadratic or cubic rows in d_spec (system s at s x spec_sys words) into d_xl, system s at
	// s x x.rows x xs
	int expand_xl_batch(const XlShape &x, i64 nsys, i64 spec_sys, i64 stride)
	{
		xs = round_up(stride, 2);
		if (int rc = alloc((void **)&d_xl, sizeof(u64) * (size_t)(nsys * x.rows * xs))) return rc;
		return enqueue_xl_expand_batch(x, d_spec, spec_sys, ss, nsys, d_xl, xs, x.rows * xs, held.st);
	}
	// `nrows` rows of the expansion (`xl`: of the XL expansion) into host memory, `stride` words apart; the host waits
	int download(void *out, i64 stride, i64 nrows, bool xl = false)
	{
		HIPCHK(hipMemcpy2DAsync(out, stride * 8, xl ? d_xl : d_aug, (xl ? xs : ds) * 8, stride * 8, nrows, hipMemcpyDeviceToHost, held.st));
		HIPCHK(hipStreamSynchronize(held.st));
		return GF2BV_OK;
	}
};

// the shape rules the two batched expansion entries share; no pointer is looked at
int check_xl_batch(XlShape &x, i64 nsys, i64 quad_sys_stride, i64 quad_stride, i64 stride, i64 sys_stride)
{
	if (nsys < 0) return fail(GF2BV_ERR_ARG, "nsys must not be negative");
	int rc = check_xl(x, quad_stride);
	if (rc) return rc;
	if (nsys * std::max<i64>(x.rows, 1) >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, "the rows of all systems together must stay below 2^31 - 64");
	if (quad_sys_stride < x.m * quad_stride)
		return fail(GF2BV_ERR_ARG, x.src == 3 ? "cubic_sys_stride_words must be at least m * cubic_stride_words"
		                                      : "quad_sys_stride_words must be at least m * quad_stride_words");
	if (stride < x.wt() || stride >= (1ll << 31)) return fail(GF2BV_ERR_ARG, "stride_words does not cover cols+1 bits");
	if (sys_stride < x.rows * stride) return fail(GF2BV_ERR_ARG, "sys_stride_words must be at least rows * stride_words");
	return GF2BV_OK;
}

// behind the rows in stage.d_aug: specialisation, batched expansion and the gang solve, all ordered on the stage's stream
int solve_guess_staged(QuadStage &stage, const GuessShape &g, int mode, int device, gf2bv_result **out)
{
	int rc = stage.specialise(g, round_up(g.x.wsrc(), 2));
	if (!rc) rc = stage.expand_xl_batch(g.x, g.na, g.m * stage.ss, g.x.wt());
	if (rc) return rc;
	rc = gf2bv_solve_batch_device(stage.d_xl, g.na, g.x.rows * stage.xs, g.x.rows, g.x.cols(), stage.xs, mode, device, stage.held.st, 0, out);
	if (rc)
		for (i64 s = 0; s < g.na; s++) { gf2bv_result_free(out[s]); out[s] = nullptr; }
	return rc;
}

}  // namespace

extern "C" {

// ---- the three entries on one factored system, quadratic or cubic (the terms say which kernel): each body once, the exported names
// behind them.  The entries on host memory null their outputs, check, stage (QuadStage) and call the device entry underneath on the
// stage's stream (the host waits only where that entry waits), or copy the expansion back
static int terms_expand_device(const Terms &t, void *d_aug, int64_t stride_words, int device, void *stream)
{
	return catching([&]() -> int {
	int rc = check_terms(t, false);
	if (rc) return rc;
	if (!d_aug) return fail(GF2BV_ERR_ARG, "null pointer");
	if (stride_words % 2 != 0 || stride_words < t.wt() || ((uintptr_t)d_aug & 15))
		return fail(GF2BV_ERR_ARG, "device matrix needs 16-byte alignment and an even stride_words covering cols+1 bits");
	rc = check_device(device);
	if (rc) return rc;
	return enqueue_expand(t, (u64 *)d_aug, stride_words, (hipStream_t)stream);
	});
}

// (nomem: what a refused pool buffer is reported as, see QuadStage)
static int terms_expand_words(const Terms &t, uint64_t *out_aug, int64_t stride_words, int device, bool nomem)
{
	return catching([&]() -> int {
	int rc = check_terms(t, true);
	if (rc) return rc;
	if (!out_aug && t.rows > 0) return fail(GF2BV_ERR_ARG, "null pointer");
	if (stride_words < t.wt()) return fail(GF2BV_ERR_ARG, "stride_words does not cover cols+1 bits");
	if ((rc = check_device(device))) return rc;
	if (t.rows == 0) return GF2BV_OK;
	QuadStage stage(device, nomem);
	if ((rc = stage.expand(t, stride_words))) return rc;
	return stage.download(out_aug, stride_words, t.rows);
	});
}

static int solve_terms(const Terms &t, int mode, int device, gf2bv_result **out, bool nomem)
{
	return catching([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	int rc = check_terms(t, true);
	if (!rc) rc = check_shape(t.rows, t.cols(), mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	QuadStage stage(device, nomem);
	if ((rc = stage.expand(t, t.wt()))) return rc;
	return gf2bv_solve_device(stage.d_aug, t.rows, t.cols(), stage.ds, mode, device, stage.held.st, 0, out);
	});
}

int gf2bv_quad_expand_device(const void *d_lin, const void *d_term_off, const void *d_ta, const void *d_tb, int64_t rows_live,
                             int64_t rows, int64_t n_lin, void *d_aug, int64_t stride_words, int device, void *stream)
{
	return terms_expand_device(Terms(d_lin, rows_live, rows, n_lin, { { d_term_off, d_ta, d_tb } }), d_aug, stride_words, device, stream);
}
int gf2bv_quad_expand_words(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t rows_live,
                            int64_t rows, int64_t n_lin, uint64_t *out_aug, int64_t stride_words, int device)
{
	return terms_expand_words(Terms(lin, rows_live, rows, n_lin, { { term_off, ta, tb } }), out_aug, stride_words, device, false);
}
int gf2bv_solve_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t rows_live,
                           int64_t rows, int64_t n_lin, int mode, int device, gf2bv_result **out)
{
	return solve_terms(Terms(lin, rows_live, rows, n_lin, { { term_off, ta, tb } }), mode, device, out, false);
}
int gf2bv_cubic_expand_device(const void *d_lin, const void *d_off2, const void *d_ta, const void *d_tb, const void *d_off3, const void *d_ua,
                              const void *d_ub, const void *d_uc, int64_t rows_live, int64_t rows, int64_t n_lin, void *d_aug,
                              int64_t stride_words, int device, void *stream)
{
	return terms_expand_device(Terms(d_lin, rows_live, rows, n_lin, { { d_off2, d_ta, d_tb }, { d_off3, d_ua, d_ub, d_uc } }), d_aug, stride_words, device, stream);
}
int gf2bv_cubic_expand_words(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                             const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, int64_t rows_live, int64_t rows, int64_t n_lin,
                             uint64_t *out_aug, int64_t stride_words, int device)
{
	return terms_expand_words(Terms(lin, rows_live, rows, n_lin, { { off2, ta, tb }, { off3, ua, ub, uc } }), out_aug, stride_words, device, true);
}
int gf2bv_solve_cubic_terms(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                            const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, int64_t rows_live, int64_t rows, int64_t n_lin,
                            int mode, int device, gf2bv_result **out)
{
	return solve_terms(Terms(lin, rows_live, rows, n_lin, { { off2, ta, tb }, { off3, ua, ub, uc } }), mode, device, out, true);
}

int gf2bv_quartic_expand_device(const void *d_lin, const void *d_off2, const void *d_ta, const void *d_tb, const void *d_off3, const void *d_ua,
                                const void *d_ub, const void *d_uc, const void *d_off4, const void *d_va, const void *d_vb, const void *d_vc,
                                const void *d_vd, int64_t rows_live, int64_t rows, int64_t n_lin, void *d_aug, int64_t stride_words, int device,
                                void *stream)
{
	return terms_expand_device(Terms(d_lin, rows_live, rows, n_lin, { { d_off2, d_ta, d_tb }, { d_off3, d_ua, d_ub, d_uc }, { d_off4, d_va, d_vb, d_vc, d_vd } }),
	                           d_aug, stride_words, device, stream);
}
int gf2bv_quartic_expand_words(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                               const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, const int64_t *off4, const uint64_t *va,
                               const uint64_t *vb, const uint64_t *vc, const uint64_t *vd, int64_t rows_live, int64_t rows, int64_t n_lin,
                               uint64_t *out_aug, int64_t stride_words, int device)
{
	return terms_expand_words(Terms(lin, rows_live, rows, n_lin, { { off2, ta, tb }, { off3, ua, ub, uc }, { off4, va, vb, vc, vd } }), out_aug, stride_words,
	                          device, true);
}
int gf2bv_solve_quartic_terms(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                              const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, const int64_t *off4, const uint64_t *va,
                              const uint64_t *vb, const uint64_t *vc, const uint64_t *vd, int64_t rows_live, int64_t rows, int64_t n_lin,
                              int mode, int device, gf2bv_result **out)
{
	return solve_terms(Terms(lin, rows_live, rows, n_lin, { { off2, ta, tb }, { off3, ua, ub, uc }, { off4, va, vb, vc, vd } }), mode, device, out, true);
}

int gf2bv_quartic_chunks(int64_t n_lin, int32_t *quad_chunk, int32_t *cubic_chunk, int32_t *quartic_chunk)
{
	return catching([&]() -> int {
	if (!quad_chunk || !cubic_chunk || !quartic_chunk) return fail(GF2BV_ERR_ARG, "null pointer");
	if (n_lin < 1 || n_lin > 65535) return fail(GF2BV_ERR_ARG, "n_lin must be 1..65535");
	const ExpandLaunch l = expand_launch(4, n_lin, 2);
	if ((i64)l.lds > kQuarticLdsBytes)
		return fail(GF2BV_ERR_ARG, "the operands and the staged cubic rows of this n_lin do not fit the expansion kernel's LDS (160 KiB)");
	*quad_chunk = l.tch[0];
	*cubic_chunk = l.tch[1];
	*quartic_chunk = l.tch[2];
	return GF2BV_OK;
	});
}

int gf2bv_cubic_chunks(int64_t n_lin, int32_t *quad_chunk, int32_t *cubic_chunk)
{
	return catching([&]() -> int {
	if (!quad_chunk || !cubic_chunk) return fail(GF2BV_ERR_ARG, "null pointer");
	if (n_lin < 1 || n_lin > 65535) return fail(GF2BV_ERR_ARG, "n_lin must be 1..65535");
	const ExpandLaunch l = expand_launch(3, n_lin, 2);
	*quad_chunk = l.tch[0];
	*cubic_chunk = l.tch[1];
	return GF2BV_OK;
	});
}

int gf2bv_factor_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t rows_live,
                            int64_t rows, int64_t n_lin, int mode, int device, gf2bv_factor **out)
{
	return catching([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	const Terms q(lin, rows_live, rows, n_lin, { { term_off, ta, tb } });
	int rc = check_terms(q, true);
	if (!rc) rc = check_shape(rows, q.cols(), mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	QuadStage stage(device);
	if ((rc = stage.expand(q, q.wt()))) return rc;
	return gf2bv_factor_device(stage.d_aug, rows, q.cols(), stage.ds, mode, device, stage.held.st, out);
	});
}

int gf2bv_factor_append_quad_terms(gf2bv_factor *h, const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb,
                                   int64_t rows, int64_t n_lin)
{
	return catching([&]() -> int {
	if (!h) return fail(GF2BV_ERR_ARG, "null pointer");
	if (h->failed) return fail(GF2BV_ERR_ARG, kFailedHandle);
	if (rows < 1) return fail(GF2BV_ERR_ARG, "rows must be at least 1");
	const Terms q(lin, rows, rows, n_lin, { { term_off, ta, tb } });
	int rc = check_terms(q, true);
	if (rc) return rc;
	if (q.cols() != h->cols) return fail(GF2BV_ERR_ARG, "n_lin does not match the handle's columns");
	if (h->rows + rows >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, "system too large");
	if ((rc = check_device(h->device))) return rc;
	// (the uploaded terms and the expansion are taken before gf2bv_factor_append_device takes its own buffers: a refusal of any
	// of them leaves the handle as it was)
	QuadStage stage(h->device);
	if ((rc = stage.expand(q, q.wt()))) return rc;
	return gf2bv_factor_append_device(h, stage.d_aug, rows, stage.ds, stage.held.st);
	});
}

int gf2bv_solve_rhs_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t rows_live,
                               int64_t rows, int64_t n_lin, const uint64_t *rhs, int64_t nrhs, int64_t rhs_words, int mode, int device,
                               gf2bv_result **out)
{
	return catching([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 j = 0; j < nrhs; j++) out[j] = nullptr;
	const Terms q(lin, rows_live, rows, n_lin, { { term_off, ta, tb } });
	int rc = check_terms(q, true);
	if (!rc) rc = check_shape(rows, q.cols(), mode);
	if (!rc) rc = check_rhs_args(rows, q.cols(), rhs, false, nrhs, rhs_words);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	QuadStage stage(device);
	if ((rc = stage.expand(q, q.wt(), nullptr, 1, reinterpret_cast<const u64 *>(rhs), sizeof(u64) * (size_t)(nrhs * rhs_words)))) return rc;
	// (the constant the expansion leaves in column `cols` is ignored there: the caller's rhs holds the constants)
	return gf2bv_solve_rhs_device(stage.d_aug, rows, q.cols(), stage.ds, stage.d_rhs, nrhs, rhs_words, mode, device, stage.held.st, 0, out);
	});
}

int gf2bv_quad_expand_batch_words(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb,
                                  const int64_t *sys_row_off, int64_t nsys, int64_t rows, int64_t n_lin, uint64_t *out_aug,
                                  int64_t stride_words, int device)
{
	return catching([&]() -> int {
	if (nsys < 0) return fail(GF2BV_ERR_ARG, "nsys must not be negative");
	const i64 *sys_off = reinterpret_cast<const i64 *>(sys_row_off);
	Terms q(lin, 0, rows, n_lin, { { term_off, ta, tb } });
	int rc = check_quad_batch(q, sys_off, nsys);
	if (rc) return rc;
	if (!out_aug && rows > 0 && nsys > 0) return fail(GF2BV_ERR_ARG, "null pointer");
	if (stride_words < q.wt()) return fail(GF2BV_ERR_ARG, "stride_words does not cover cols+1 bits");
	if ((rc = check_device(device))) return rc;
	if (rows == 0 || nsys == 0) return GF2BV_OK;
	QuadStage stage(device);
	if ((rc = stage.expand(q, stride_words, sys_off, nsys))) return rc;
	return stage.download(out_aug, stride_words, nsys * rows);
	});
}

int gf2bv_solve_batch_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb,
                                 const int64_t *sys_row_off, int64_t nsys, int64_t rows, int64_t n_lin, int mode, int device,
                                 gf2bv_result **out)
{
	return catching([&]() -> int {
	if (!out || nsys < 0) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 s = 0; s < nsys; s++) out[s] = nullptr;
	const i64 *sys_off = reinterpret_cast<const i64 *>(sys_row_off);
	Terms q(lin, 0, rows, n_lin, { { term_off, ta, tb } });
	int rc = check_quad_batch(q, sys_off, nsys);
	if (!rc) rc = check_shape(rows, q.cols(), mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	if (nsys == 0) return GF2BV_OK;
	QuadStage stage(device);
	if ((rc = stage.expand(q, q.wt(), sys_off, nsys))) return rc;
	// (the gangs run on streams of their own, behind an event gf2bv_solve_batch_device records on this one)
	return gf2bv_solve_batch_device(stage.d_aug, nsys, rows * stage.ds, rows, q.cols(), stage.ds, mode, device, stage.held.st, 0, out);
	});
}

// ---- degree-3 XL: the quadratic rows (expanded already, or factored) multiplied by 1 and by every unknown on the device
// (src: the degree of the source rows -- 2 everywhere but in the gf2bv_*_xl4_cubic_* entries at the end, whose rows are cubic)
static int xl_expand_device(int degree, int src, const void *d_quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, void *d_aug,
                            int64_t stride_words, int device, void *stream)
{
	return catching([&]() -> int {
	XlShape x(degree, src, m, n_lin, rows);
	if (!d_aug || (!d_quad && m > 0)) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_xl(x, quad_stride_words);
	if (rc) return rc;
	if (stride_words % 2 != 0 || stride_words < x.wt() || ((uintptr_t)d_aug & 15))
		return fail(GF2BV_ERR_ARG, "device matrix needs 16-byte alignment and an even stride_words covering cols+1 bits");
	if ((rc = check_device(device))) return rc;
	return enqueue_xl_expand(x, (const u64 *)d_quad, quad_stride_words, (u64 *)d_aug, stride_words, (hipStream_t)stream);
	});
}

static int xl_expand_words(int degree, int src, const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, uint64_t *out_aug,
                           int64_t stride_words, int device)
{
	return catching([&]() -> int {
	XlShape x(degree, src, m, n_lin, rows);
	if ((!out_aug && rows > 0) || (!quad && m > 0)) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_xl(x, quad_stride_words);
	if (rc) return rc;
	if (stride_words < x.wt()) return fail(GF2BV_ERR_ARG, "stride_words does not cover cols+1 bits");
	if ((rc = check_device(device))) return rc;
	if (rows == 0) return GF2BV_OK;
	QuadStage stage(device);
	if ((rc = stage.upload_rows(reinterpret_cast<const u64 *>(quad), m, quad_stride_words))) return rc;
	if ((rc = stage.expand_xl(x, stride_words))) return rc;
	return stage.download(out_aug, stride_words, rows, true);
	});
}

static int solve_xl_words(int degree, int src, const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int mode, int device,
                          gf2bv_result **out)
{
	return catching([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	if (!quad && m > 0) return fail(GF2BV_ERR_ARG, "null pointer");
	XlShape x(degree, src, m, n_lin);
	int rc = check_xl(x, quad_stride_words, true);
	if (!rc) rc = check_shape(x.rows, x.cols(), mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	QuadStage stage(device);
	if ((rc = stage.upload_rows(reinterpret_cast<const u64 *>(quad), m, quad_stride_words))) return rc;
	if ((rc = stage.expand_xl(x, x.wt()))) return rc;
	return gf2bv_solve_device(stage.d_xl, x.rows, x.cols(), stage.xs, mode, device, stage.held.st, 0, out);
	});
}

// (the factored form of either degree: t.rows = t.rows_live = m rows, no padding, expanded by its own kernel in front of the XL kernel)
static int solve_xl_terms(int degree, const Terms &t, int mode, int device, gf2bv_result **out)
{
	return catching([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	*out = nullptr;
	int rc = check_terms(t, true);
	if (rc) return rc;
	XlShape x(degree, t.degree(), t.rows, t.n);
	rc = check_xl(x, t.wt(), true);
	if (!rc) rc = check_shape(x.rows, x.cols(), mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	QuadStage stage(device);
	if ((rc = stage.expand(t, t.wt()))) return rc;
	if ((rc = stage.expand_xl(x, x.wt()))) return rc;
	return gf2bv_solve_device(stage.d_xl, x.rows, x.cols(), stage.xs, mode, device, stage.held.st, 0, out);
	});
}

// ---- hybrid XL: guessed unknowns substituted for many assignments at once, every assignment's system expanded and solved as one batch
// (src: the degree of the source rows -- 2 everywhere but in the gf2bv_*_cubic_* entries at the end, whose rows are cubic)
static int specialise_device(int src, const void *d_quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                             int64_t nguess, int64_t a0, int64_t na, void *d_out, int64_t out_stride_words, int64_t sys_stride_words,
                             int device, void *stream)
{
	return catching([&]() -> int {
	GuessShape g(m, n_lin, nguess, a0, na, src + 1, src);
	if (!d_out || (!d_quad && m > 0)) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_guess(g, guess, quad_stride_words);
	if (rc) return rc;
	if (out_stride_words < g.x.wsrc() || out_stride_words >= (1ll << 31) || sys_stride_words < m * out_stride_words || ((uintptr_t)d_out & 7))
		return fail(GF2BV_ERR_ARG, "out_stride_words must cover the specialised columns and the constant, sys_stride_words m rows of it");
	if ((rc = check_device(device))) return rc;
	return enqueue_specialise(g, (const u64 *)d_quad, quad_stride_words, (u64 *)d_out, out_stride_words, sys_stride_words, (hipStream_t)stream);
	});
}

static int specialise_words(int src, const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                            int64_t nguess, int64_t a0, int64_t na, uint64_t *out, int64_t out_stride_words, int device)
{
	return catching([&]() -> int {
	GuessShape g(m, n_lin, nguess, a0, na, src + 1, src);
	if ((!out && m > 0 && na > 0) || (!quad && m > 0)) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_guess(g, guess, quad_stride_words);
	if (rc) return rc;
	if (out_stride_words < g.x.wsrc() || out_stride_words >= (1ll << 31))
		return fail(GF2BV_ERR_ARG, "out_stride_words does not cover the specialised columns and the constant");
	if ((rc = check_device(device))) return rc;
	if (m == 0 || na == 0) return GF2BV_OK;
	QuadStage stage(device);
	if ((rc = stage.upload_rows(reinterpret_cast<const u64 *>(quad), m, quad_stride_words))) return rc;
	if ((rc = stage.specialise(g, out_stride_words))) return rc;          // (the caller's stride, odd or even: the rows come back as they are)
	HIPCHK(hipMemcpyAsync(out, stage.d_spec, sizeof(u64) * (size_t)(na * m * out_stride_words), hipMemcpyDeviceToHost, stage.held.st));
	HIPCHK(hipStreamSynchronize(stage.held.st));
	return GF2BV_OK;
	});
}

static int xl_expand_batch_device(int degree, int src, const void *d_quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                  int64_t n_lin, int64_t rows, void *d_aug, int64_t stride_words, int64_t sys_stride_words, int device,
                                  void *stream)
{
	return catching([&]() -> int {
	XlShape x(degree, src, m, n_lin, rows);
	if (!d_aug || (!d_quad && m > 0)) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_xl_batch(x, nsys, quad_sys_stride_words, quad_stride_words, stride_words, sys_stride_words);
	if (rc) return rc;
	if (stride_words % 2 != 0 || sys_stride_words % 2 != 0 || ((uintptr_t)d_aug & 15))
		return fail(GF2BV_ERR_ARG, "device matrices need 16-byte alignment and even stride_words and sys_stride_words");
	if ((rc = check_device(device))) return rc;
	return enqueue_xl_expand_batch(x, (const u64 *)d_quad, quad_sys_stride_words, quad_stride_words, nsys, (u64 *)d_aug, stride_words,
	                                sys_stride_words, (hipStream_t)stream);
	});
}

static int xl_expand_batch_words(int degree, int src, const uint64_t *quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                 int64_t n_lin, int64_t rows, uint64_t *out_aug, int64_t stride_words, int64_t sys_stride_words, int device)
{
	return catching([&]() -> int {
	XlShape x(degree, src, m, n_lin, rows);
	if ((!out_aug && rows > 0 && nsys > 0) || (!quad && m > 0 && nsys > 0)) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_xl_batch(x, nsys, quad_sys_stride_words, quad_stride_words, stride_words, sys_stride_words);
	if (rc) return rc;
	if ((rc = check_device(device))) return rc;
	if (rows == 0 || nsys == 0) return GF2BV_OK;
	QuadStage stage(device);
	if ((rc = stage.open())) return rc;
	stage.ss = quad_stride_words;                      // (the last system's rows end the source: nothing behind them is read)
	if ((rc = stage.upload(&stage.d_spec, reinterpret_cast<const u64 *>(quad),
	                       m ? sizeof(u64) * (size_t)((nsys - 1) * quad_sys_stride_words + m * quad_stride_words) : 0))) return rc;
	if ((rc = stage.expand_xl_batch(x, nsys, quad_sys_stride_words, stride_words))) return rc;
	if (sys_stride_words == rows * stride_words)
		HIPCHK(hipMemcpy2DAsync(out_aug, stride_words * 8, stage.d_xl, stage.xs * 8, stride_words * 8, nsys * rows, hipMemcpyDeviceToHost, stage.held.st));
	else
		for (i64 s = 0; s < nsys; s++)
			HIPCHK(hipMemcpy2DAsync(out_aug + s * sys_stride_words, stride_words * 8, stage.d_xl + s * rows * stage.xs, stage.xs * 8,
			                        stride_words * 8, rows, hipMemcpyDeviceToHost, stage.held.st));
	HIPCHK(hipStreamSynchronize(stage.held.st));
	return GF2BV_OK;
	});
}

static int solve_xl_guess_words(int degree, int src, const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                                int64_t nguess, int64_t a0, int64_t na, int mode, int device, gf2bv_result **out)
{
	return catching([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 s = 0; s < na; s++) out[s] = nullptr;
	if (!quad && m > 0) return fail(GF2BV_ERR_ARG, "null pointer");
	GuessShape g(m, n_lin, nguess, a0, na, degree, src);
	int rc = check_guess(g, guess, quad_stride_words);
	if (!rc) rc = check_guess_solve(g, mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	if (na == 0) return GF2BV_OK;
	QuadStage stage(device);
	if ((rc = stage.upload_rows(reinterpret_cast<const u64 *>(quad), m, quad_stride_words))) return rc;
	return solve_guess_staged(stage, g, mode, device, out);
	});
}

// (the factored form of either degree: q.rows = q.rows_live = m rows, no padding)
static int solve_xl_guess_terms(int degree, const Terms &q, const int32_t *guess, int64_t nguess, int64_t a0, int64_t na, int mode, int device,
                                gf2bv_result **out)
{
	return catching([&]() -> int {
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	for (i64 s = 0; s < na; s++) out[s] = nullptr;
	int rc = check_terms(q, true);
	if (rc) return rc;
	GuessShape g(q.rows, q.n, nguess, a0, na, degree, q.degree());
	rc = check_guess(g, guess, q.wt());
	if (!rc) rc = check_guess_solve(g, mode);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	if (na == 0) return GF2BV_OK;
	QuadStage stage(device);
	if ((rc = stage.expand(q, q.wt()))) return rc;
	return solve_guess_staged(stage, g, mode, device, out);
	});
}

// The largest number of assignments (at most 2^nguess) whose specialised rows and padded expansions take at most a quarter of
// free_bytes -- the solver keeps a tile-major copy of about the size of every system of a gang, so expansion and copy stay below half of
// what was free -- and whose rows together stay below 2^31 - 64; 0 when one system does not fit, -1 for a bad shape.  No device is touched.
static int64_t xl_guess_chunk(int degree, int src, int64_t m, int64_t n_lin, int64_t nguess, int64_t free_bytes)
{
	if (n_lin < 1 || n_lin > 65535 || nguess < 0 || nguess > std::min<i64>(n_lin - 1, 30) || m < 0 || free_bytes < 0) return -1;
	XlShape x(degree, src, m, n_lin - nguess);
	if (check_xl(x, x.wsrc(), true)) return -1;
	const i64 fit = free_bytes / 4 / guess_system_bytes(x);
	return std::min<i64>({ 1ll << nguess, fit, ((1ll << 31) - 65) / x.rows });
}

static int xl_guess_chunk_device(int degree, int src, int64_t m, int64_t n_lin, int64_t nguess, int device, int64_t *chunk)
{
	return catching([&]() -> int {
	if (!chunk) return fail(GF2BV_ERR_ARG, "null pointer");
	*chunk = 0;
	if (xl_guess_chunk(degree, src, m, n_lin, nguess, 0) < 0) return fail(GF2BV_ERR_ARG, "m, n_lin or nguess out of range");
	int rc = check_device(device);
	if (rc) return rc;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	HIPCHK(hipMemGetInfo(&free_b, &total_b));
	// (what the pool holds idle is handed out again before the device is asked for more)
	*chunk = xl_guess_chunk(degree, src, m, n_lin, nguess, (i64)free_b + std::max<i64>(0, gf2bv_pool_idle_bytes(device)));
	return GF2BV_OK;
	});
}

// the exported names: each body above once, for degree 3 and degree 4
int gf2bv_quad_specialise_device(const void *d_quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                                 int64_t nguess, int64_t a0, int64_t na, void *d_out, int64_t out_stride_words, int64_t sys_stride_words,
                                 int device, void *stream)
{
	return specialise_device(2, d_quad, m, quad_stride_words, n_lin, guess, nguess, a0, na, d_out, out_stride_words, sys_stride_words, device, stream);
}
int gf2bv_quad_specialise_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                                int64_t nguess, int64_t a0, int64_t na, uint64_t *out, int64_t out_stride_words, int device)
{
	return specialise_words(2, quad, m, quad_stride_words, n_lin, guess, nguess, a0, na, out, out_stride_words, device);
}
int gf2bv_xl3_expand_device(const void *d_quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, void *d_aug,
                            int64_t stride_words, int device, void *stream)
{
	return xl_expand_device(3, 2, d_quad, m, quad_stride_words, n_lin, rows, d_aug, stride_words, device, stream);
}
int gf2bv_xl4_expand_device(const void *d_quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, void *d_aug,
                            int64_t stride_words, int device, void *stream)
{
	return xl_expand_device(4, 2, d_quad, m, quad_stride_words, n_lin, rows, d_aug, stride_words, device, stream);
}
int gf2bv_xl3_expand_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, uint64_t *out_aug,
                           int64_t stride_words, int device)
{
	return xl_expand_words(3, 2, quad, m, quad_stride_words, n_lin, rows, out_aug, stride_words, device);
}
int gf2bv_xl4_expand_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, uint64_t *out_aug,
                           int64_t stride_words, int device)
{
	return xl_expand_words(4, 2, quad, m, quad_stride_words, n_lin, rows, out_aug, stride_words, device);
}
int gf2bv_solve_xl3_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int mode, int device, gf2bv_result **out)
{
	return solve_xl_words(3, 2, quad, m, quad_stride_words, n_lin, mode, device, out);
}
int gf2bv_solve_xl4_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int mode, int device, gf2bv_result **out)
{
	return solve_xl_words(4, 2, quad, m, quad_stride_words, n_lin, mode, device, out);
}
int gf2bv_solve_xl3_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t m, int64_t n_lin,
                               int mode, int device, gf2bv_result **out)
{
	return solve_xl_terms(3, Terms(lin, m, m, n_lin, { { term_off, ta, tb } }), mode, device, out);
}
int gf2bv_solve_xl4_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t m, int64_t n_lin,
                               int mode, int device, gf2bv_result **out)
{
	return solve_xl_terms(4, Terms(lin, m, m, n_lin, { { term_off, ta, tb } }), mode, device, out);
}
int gf2bv_xl3_expand_batch_device(const void *d_quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                  int64_t n_lin, int64_t rows, void *d_aug, int64_t stride_words, int64_t sys_stride_words, int device,
                                  void *stream)
{
	return xl_expand_batch_device(3, 2, d_quad, nsys, quad_sys_stride_words, m, quad_stride_words, n_lin, rows, d_aug, stride_words, sys_stride_words,
	                              device, stream);
}
int gf2bv_xl4_expand_batch_device(const void *d_quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                  int64_t n_lin, int64_t rows, void *d_aug, int64_t stride_words, int64_t sys_stride_words, int device,
                                  void *stream)
{
	return xl_expand_batch_device(4, 2, d_quad, nsys, quad_sys_stride_words, m, quad_stride_words, n_lin, rows, d_aug, stride_words, sys_stride_words,
	                              device, stream);
}
int gf2bv_xl3_expand_batch_words(const uint64_t *quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                 int64_t n_lin, int64_t rows, uint64_t *out_aug, int64_t stride_words, int64_t sys_stride_words, int device)
{
	return xl_expand_batch_words(3, 2, quad, nsys, quad_sys_stride_words, m, quad_stride_words, n_lin, rows, out_aug, stride_words, sys_stride_words,
	                             device);
}
int gf2bv_xl4_expand_batch_words(const uint64_t *quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                 int64_t n_lin, int64_t rows, uint64_t *out_aug, int64_t stride_words, int64_t sys_stride_words, int device)
{
	return xl_expand_batch_words(4, 2, quad, nsys, quad_sys_stride_words, m, quad_stride_words, n_lin, rows, out_aug, stride_words, sys_stride_words,
	                             device);
}
int gf2bv_solve_xl3_guess_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess, int64_t nguess,
                                int64_t a0, int64_t na, int mode, int device, gf2bv_result **out)
{
	return solve_xl_guess_words(3, 2, quad, m, quad_stride_words, n_lin, guess, nguess, a0, na, mode, device, out);
}
int gf2bv_solve_xl4_guess_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess, int64_t nguess,
                                int64_t a0, int64_t na, int mode, int device, gf2bv_result **out)
{
	return solve_xl_guess_words(4, 2, quad, m, quad_stride_words, n_lin, guess, nguess, a0, na, mode, device, out);
}
int gf2bv_solve_xl3_guess_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t m, int64_t n_lin,
                                     const int32_t *guess, int64_t nguess, int64_t a0, int64_t na, int mode, int device, gf2bv_result **out)
{
	return solve_xl_guess_terms(3, Terms(lin, m, m, n_lin, { { term_off, ta, tb } }), guess, nguess, a0, na, mode, device, out);
}
int gf2bv_solve_xl4_guess_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t m, int64_t n_lin,
                                     const int32_t *guess, int64_t nguess, int64_t a0, int64_t na, int mode, int device, gf2bv_result **out)
{
	return solve_xl_guess_terms(4, Terms(lin, m, m, n_lin, { { term_off, ta, tb } }), guess, nguess, a0, na, mode, device, out);
}
int64_t gf2bv_xl3_guess_chunk(int64_t m, int64_t n_lin, int64_t nguess, int64_t free_bytes)
{
	return xl_guess_chunk(3, 2, m, n_lin, nguess, free_bytes);
}
int64_t gf2bv_xl4_guess_chunk(int64_t m, int64_t n_lin, int64_t nguess, int64_t free_bytes)
{
	return xl_guess_chunk(4, 2, m, n_lin, nguess, free_bytes);
}
int gf2bv_xl3_guess_chunk_device(int64_t m, int64_t n_lin, int64_t nguess, int device, int64_t *chunk)
{
	return xl_guess_chunk_device(3, 2, m, n_lin, nguess, device, chunk);
}
int gf2bv_xl4_guess_chunk_device(int64_t m, int64_t n_lin, int64_t nguess, int device, int64_t *chunk)
{
	return xl_guess_chunk_device(4, 2, m, n_lin, nguess, device, chunk);
}

// ---- degree-4 XL on cubic rows (k_xl4_cubic_expand): the bodies above with src = 3, and the factored form staged through both kernels
int gf2bv_xl4_cubic_expand_device(const void *d_cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, int64_t rows, void *d_aug,
                                  int64_t stride_words, int device, void *stream)
{
	return xl_expand_device(4, 3, d_cubic, m, cubic_stride_words, n_lin, rows, d_aug, stride_words, device, stream);
}
int gf2bv_xl4_cubic_expand_words(const uint64_t *cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, int64_t rows, uint64_t *out_aug,
                                 int64_t stride_words, int device)
{
	return xl_expand_words(4, 3, cubic, m, cubic_stride_words, n_lin, rows, out_aug, stride_words, device);
}
int gf2bv_solve_xl4_cubic_words(const uint64_t *cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, int mode, int device,
                                gf2bv_result **out)
{
	return solve_xl_words(4, 3, cubic, m, cubic_stride_words, n_lin, mode, device, out);
}
int gf2bv_solve_xl4_cubic_terms(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                                const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, int64_t m, int64_t n_lin, int mode, int device,
                                gf2bv_result **out)
{
	return solve_xl_terms(4, Terms(lin, m, m, n_lin, { { off2, ta, tb }, { off3, ua, ub, uc } }), mode, device, out);
}

// ---- hybrid degree-4 XL on cubic rows (k_cubic_specialise, k_xl4_cubic_expand_batch): the hybrid bodies above with src = 3
int gf2bv_cubic_specialise_device(const void *d_cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, const int32_t *guess,
                                  int64_t nguess, int64_t a0, int64_t na, void *d_out, int64_t out_stride_words, int64_t sys_stride_words,
                                  int device, void *stream)
{
	return specialise_device(3, d_cubic, m, cubic_stride_words, n_lin, guess, nguess, a0, na, d_out, out_stride_words, sys_stride_words, device, stream);
}
int gf2bv_cubic_specialise_words(const uint64_t *cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, const int32_t *guess,
                                 int64_t nguess, int64_t a0, int64_t na, uint64_t *out, int64_t out_stride_words, int device)
{
	return specialise_words(3, cubic, m, cubic_stride_words, n_lin, guess, nguess, a0, na, out, out_stride_words, device);
}
int gf2bv_xl4_cubic_expand_batch_device(const void *d_cubic, int64_t nsys, int64_t cubic_sys_stride_words, int64_t m, int64_t cubic_stride_words,
                                        int64_t n_lin, int64_t rows, void *d_aug, int64_t stride_words, int64_t sys_stride_words, int device,
                                        void *stream)
{
	return xl_expand_batch_device(4, 3, d_cubic, nsys, cubic_sys_stride_words, m, cubic_stride_words, n_lin, rows, d_aug, stride_words,
	                              sys_stride_words, device, stream);
}
int gf2bv_xl4_cubic_expand_batch_words(const uint64_t *cubic, int64_t nsys, int64_t cubic_sys_stride_words, int64_t m, int64_t cubic_stride_words,
                                       int64_t n_lin, int64_t rows, uint64_t *out_aug, int64_t stride_words, int64_t sys_stride_words, int device)
{
	return xl_expand_batch_words(4, 3, cubic, nsys, cubic_sys_stride_words, m, cubic_stride_words, n_lin, rows, out_aug, stride_words,
	                             sys_stride_words, device);
}
int gf2bv_solve_xl4_cubic_guess_words(const uint64_t *cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, const int32_t *guess,
                                      int64_t nguess, int64_t a0, int64_t na, int mode, int device, gf2bv_result **out)
{
	return solve_xl_guess_words(4, 3, cubic, m, cubic_stride_words, n_lin, guess, nguess, a0, na, mode, device, out);
}
int gf2bv_solve_xl4_cubic_guess_terms(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                                      const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, int64_t m, int64_t n_lin,
                                      const int32_t *guess, int64_t nguess, int64_t a0, int64_t na, int mode, int device, gf2bv_result **out)
{
	return solve_xl_guess_terms(4, Terms(lin, m, m, n_lin, { { off2, ta, tb }, { off3, ua, ub, uc } }), guess, nguess, a0, na, mode, device, out);
}
int64_t gf2bv_xl4_cubic_guess_chunk(int64_t m, int64_t n_lin, int64_t nguess, int64_t free_bytes)
{
	return xl_guess_chunk(4, 3, m, n_lin, nguess, free_bytes);
}
int gf2bv_xl4_cubic_guess_chunk_device(int64_t m, int64_t n_lin, int64_t nguess, int device, int64_t *chunk)
{
	return xl_guess_chunk_device(4, 3, m, n_lin, nguess, device, chunk);
}

// k_xl4_expand's quartic root, the same function compiled for the host: the largest i >= 3 with C(i,4) <= u (u >= 0), for checks
int64_t gf2bv_xl4_quartic_root(int64_t u) { return u < 0 ? -1 : xl_quart_root(u); }

}  // extern "C"

// ---- composition: affine maps substituted into affine forms, and powers of a self-map (k_compose) -------------------------------
namespace {

struct ComposeTimes { double upload = 0, kernels = 0, download = 0; i64 products = 0; };
thread_local ComposeTimes g_compose_times;

inline i64 form_words(i64 unknowns) { return (unknowns + 1 + 63) / 64; }

// ra forms over n unknowns into images over nb unknowns: the rules every entry shares; no pointer is looked at
int check_compose(i64 ra, i64 n, i64 nb)
{
	if (ra < 0) return fail(GF2BV_ERR_ARG, "ra must not be negative");
	if (n < 1 || nb < 1) return fail(GF2BV_ERR_ARG, "n and nb must be at least 1");
	if (n + 1 >= (1ll << 31) - 64 || nb + 1 >= (1ll << 31) - 64) return fail(GF2BV_ERR_ARG, "n + 1 and nb + 1 must stay below 2^31 - 64");
	const i64 tiles = (form_words(nb) + GF2_TW - 1) / GF2_TW, groups = (std::max<i64>(ra, 1) + GF2_CMP_RG - 1) / GF2_CMP_RG;
	if (tiles * groups >= (1ll << 31)) return fail(GF2BV_ERR_ARG, "column tiles x row groups of the product must stay below 2^31");
	return GF2BV_OK;
}

// a device matrix of the device entries: 16-byte aligned, an even stride that covers the width
int check_device_rows(const void *p, i64 stride, i64 width, const char *what)
{
	if (stride % 2 != 0 || stride < width || ((uintptr_t)p & 15)) return fail(GF2BV_ERR_ARG, what);
	return GF2BV_OK;
}

// (device pointers, already checked) one product on `st`: d_b is the n image rows, the kernel supplies the unit row
int enqueue_compose(const u64 *d_a, i64 ra, i64 a_stride, i64 n, const u64 *d_b, i64 b_stride, i64 nb, u64 *d_out, i64 out_stride, hipStream_t st)
{
	if (ra == 0) return GF2BV_OK;
	const i64 tiles = (form_words(nb) + GF2_TW - 1) / GF2_TW, groups = (ra + GF2_CMP_RG - 1) / GF2_CMP_RG;
	hipLaunchKernelGGL(k_compose, dim3((unsigned)(tiles * groups)), dim3(GF2_CMP_NT), 0, st, d_a, ra, a_stride, n, d_b, b_stride, nb, d_out,
	                   out_stride, tiles);
	HIPCHK(hipGetLastError());
	g_compose_times.products++;
	return GF2BV_OK;
}

int enqueue_identity(u64 *d_out, i64 rows, i64 stride, i64 first, hipStream_t st)
{
	const unsigned blocks = (unsigned)std::min<i64>((rows * stride + 255) / 256, 4096);
	hipLaunchKernelGGL(k_compose_identity, dim3(blocks), dim3(256), 0, st, d_out, rows, stride, first);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// The buffers and the stream of an entry that stages: a refused buffer is GF2BV_ERR_NOMEM, and everything goes back by the holder's rule
struct ComposeStage {
	Held held;                         // its stream: the pool's, or the caller's
	hipEvent_t ev[4] = {};
	explicit ComposeStage(int device) : held(device) {}
	int open(hipStream_t given, bool own)
	{
		if (own) HIPCHK(held.stream(0)); else held.on(given);
		for (hipEvent_t &e : ev) HIPCHK(held.event(&e));
		return GF2BV_OK;
	}
	int alloc(u64 **out, i64 words)
	{
		return held.alloc((void **)out, sizeof(u64) * (size_t)words, "the forms, the images or the product do not fit on the device", "composition buffers");
	}
	int mark(int i) { HIPCHK(hipEventRecord(ev[i], held.st)); return GF2BV_OK; }
	// after the stream has been synchronised: the times between the four marks
	int times()
	{
		float up = 0, ke = 0, dn = 0;
		HIPCHK(hipEventElapsedTime(&up, ev[0], ev[1]));
		HIPCHK(hipEventElapsedTime(&ke, ev[1], ev[2]));
		HIPCHK(hipEventElapsedTime(&dn, ev[2], ev[3]));
		g_compose_times.upload = up; g_compose_times.kernels = ke; g_compose_times.download = dn;
		return GF2BV_OK;
	}
};

// host rows `stride` words apart <-> device rows `ds` words apart, `width` words of each
int copy_rows(void *dst, i64 dst_stride, const void *src, i64 src_stride, i64 width, i64 rows, hipMemcpyKind kind, hipStream_t st)
{
	if (rows == 0) return GF2BV_OK;
	HIPCHK(hipMemcpy2DAsync(dst, (size_t)dst_stride * 8, src, (size_t)src_stride * 8, (size_t)width * 8, (size_t)rows, kind, st));
	return GF2BV_OK;
}

// Square-and-multiply on the device, most significant bit first.  d_base: the n image rows of the map, bs words apart.  cur, tmp:
// (n + 1) x ws words each, B~ of the running power with its unit row (the products write it: the unit row of A selects the unit row).
// The running power starts as the identity; a set bit multiplies by the base (the first one: identity o base, which also drops the
// base's bits above n), every later bit squares first: bit_length - 1 + popcount products, none for k = 0.  The LAST product writes
// rows 1 .. n straight to d_out (os words apart); k = 0 writes the identity's there.  d_out null: the result stays in the buffer the
// last product does not read, rows ws words apart, and *where says where.
int enqueue_power(const u64 *d_base, i64 bs, i64 n, const uint64_t *k, i64 knw, u64 *cur, u64 *tmp, i64 ws, u64 *d_out, i64 os, hipStream_t st,
                  const u64 **where = nullptr)
{
	i64 top = -1, pop = 0;
	for (i64 i = 0; i < 64 * knw; i++)
		if ((k[i >> 6] >> (i & 63)) & 1) { top = i; pop++; }
	i64 left = top < 0 ? 0 : top + pop;
	const bool stay = !d_out;
	if (stay) { d_out = tmp + ws; os = ws; }
	if (where) *where = d_out;
	if (left == 0) return enqueue_identity(d_out, n, os, 1, st);
	int rc = enqueue_identity(cur, n + 1, ws, 0, st);
	auto product = [&](const u64 *b, i64 b_stride) {
		if (rc) return;
		if (--left == 0) {
			if (stay) d_out = tmp + ws;
			if (where) *where = d_out;
			rc = enqueue_compose(cur + ws, n, ws, n, b, b_stride, n, d_out, os, st);
		}
		else { rc = enqueue_compose(cur, n + 1, ws, n, b, b_stride, n, tmp, ws, st); std::swap(cur, tmp); }
	};
	for (i64 i = top; i >= 0; i--) {
		if (i < top) product(cur + ws, ws);
		if ((k[i >> 6] >> (i & 63)) & 1) product(d_base, bs);
	}
	return rc;
}

int check_power(const void *b, i64 b_stride, i64 n, const uint64_t *k, i64 knw, const void *out, i64 out_stride)
{
	if (!b || !k || !out) return fail(GF2BV_ERR_ARG, "null pointer");
	if (knw < 1) return fail(GF2BV_ERR_ARG, "k_nwords must be at least 1");
	if (int rc = check_compose(n + 1, n, n)) return rc;
	if (b_stride < form_words(n) || out_stride < form_words(n)) return fail(GF2BV_ERR_ARG, "a stride does not cover n + 1 bits");
	return GF2BV_OK;
}

bool words_are_zero(const uint64_t *k, i64 knw)
{
	for (i64 i = 0; i < knw; i++) if (k[i]) return false;
	return true;
}

// the time steps of the largest block of the doubling schedule: block h holds min(h, count - h) of them
i64 unroll_largest_block(i64 count)
{
	i64 big = count > 0 ? 1 : 0;
	for (i64 h = 1; h < count; h *= 2) big = std::max(big, std::min(h, count - h));
	return big;
}

int check_unroll(const void *a, i64 ra, i64 a_stride, i64 n, const void *b, i64 b_stride, const uint64_t *start, i64 snw, const uint64_t *step,
                 i64 pnw, i64 count, const void *out, i64 out_stride)
{
	if (!a || !b || !start || !step || !out) return fail(GF2BV_ERR_ARG, "null pointer");
	if (count < 0) return fail(GF2BV_ERR_ARG, "count must not be negative");
	if (snw < 1 || pnw < 1) return fail(GF2BV_ERR_ARG, "start_nwords and step_nwords must be at least 1");
	if (int rc = check_compose(ra, n, n)) return rc;
	if (int rc = check_compose(n + 1, n, n)) return rc;
	if (words_are_zero(step, pnw)) return fail(GF2BV_ERR_ARG, "step must be at least 1");
	if (a_stride < form_words(n) || b_stride < form_words(n) || out_stride < form_words(n)) return fail(GF2BV_ERR_ARG, "a stride does not cover n + 1 bits");
	if (ra > 0 && count > 0) {
		// the products read and write blocks of whole time steps: the largest one has to be a legal product, and the rows one allocation
		if (count > (1ll << 62) / ra) return fail(GF2BV_ERR_ARG, "count x ra is beyond what one product can take");
		if (int rc = check_compose(unroll_largest_block(count) * ra, n, n)) return rc;
		if (count * ra > (1ll << 59) / out_stride) return fail(GF2BV_ERR_ARG, "count x ra rows of out_stride words are beyond the address space");
	}
	return GF2BV_OK;
}

int enqueue_copy(const u64 *d_src, i64 src_stride, u64 *d_dst, i64 dst_stride, i64 rows, i64 n, hipStream_t st)
{
	if (rows == 0) return GF2BV_OK;
	const unsigned blocks = (unsigned)std::min<i64>((rows * dst_stride + 255) / 256, 4096);
	hipLaunchKernelGGL(k_compose_copy, dim3(blocks), dim3(256), 0, st, d_src, src_stride, d_dst, dst_stride, rows, n);
	HIPCHK(hipGetLastError());
	return GF2BV_OK;
}

// The unrolling schedule on `st`, everything resident (device pointers, already checked; ra >= 1, count >= 1).  base, cur, tmp: power's
// three (n + 1) x ws buffers, the map's n rows at base + ws.  d_out: count x ra rows, os words apart, time-major.
//   block 0 = a o b^start: start = 0 a masked copy of a (no product); otherwise b^start by enqueue_power and one product.  It comes
//     first because enqueue_power needs both work buffers beside the base, and the step map below stays in one of them;
//   S = b^step by enqueue_power (step = 1: b where it lies, no product);
//   doubling, P = S, h = 1: rows of the times [h, min(2h, count)) = rows of the times [0, min(h, count - h)) o P, read from and written
//     to d_out -- a block is whole time steps, so the rows of a product land time-major where they belong and nothing is reordered --
//     then P = P o P into a buffer that P is not in, unless this was the last block.
// The product kernel zeroes the words between a row's last tile and its stride, the copy kernel does the same.
int enqueue_unroll(const u64 *d_a, i64 ra, i64 as, i64 n, u64 *base, u64 *cur, u64 *tmp, i64 ws, const uint64_t *start, i64 snw,
                   const uint64_t *step, i64 pnw, i64 count, u64 *d_out, i64 os, hipStream_t st)
{
	int rc;
	if (words_are_zero(start, snw)) { if ((rc = enqueue_copy(d_a, as, d_out, os, ra, n, st))) return rc; }
	else {
		const u64 *at = nullptr;
		if ((rc = enqueue_power(base + ws, ws, n, start, snw, cur, tmp, ws, nullptr, 0, st, &at))) return rc;
		if ((rc = enqueue_compose(d_a, ra, as, n, at, ws, n, d_out, os, st))) return rc;
	}
	const u64 *P = base + ws;
	u64 *other = cur;                              // a buffer that P is not in
	const bool unit_step = step[0] == 1 && words_are_zero(step + 1, pnw - 1);
	if (!unit_step) {
		if ((rc = enqueue_power(base + ws, ws, n, step, pnw, cur, tmp, ws, nullptr, 0, st, &P))) return rc;
		other = P == cur + ws ? tmp : cur;
	}
	for (i64 h = 1; h < count; h *= 2) {
		const i64 steps = std::min(h, count - h);
		if ((rc = enqueue_compose(d_out, steps * ra, os, n, P, ws, n, d_out + h * ra * os, os, st))) return rc;
		if (2 * h >= count) break;
		if ((rc = enqueue_compose(P, n, ws, n, P, ws, n, other + ws, ws, st))) return rc;
		u64 *was = const_cast<u64 *>(P) - ws;
		P = other + ws;
		other = was;
	}
	return GF2BV_OK;
}

}  // namespace

extern "C" {

int gf2bv_compose_shape(int32_t out[4])
{
	if (!out) return fail(GF2BV_ERR_ARG, "null pointer");
	out[0] = GF2_CMP_S; out[1] = GF2_CMP_RG; out[2] = GF2_TW; out[3] = GF2_CMP_LDS;
	return GF2BV_OK;
}

void gf2bv_compose_last_times(double ms[4])
{
	const ComposeTimes &t = g_compose_times;
	ms[0] = t.upload; ms[1] = t.kernels; ms[2] = t.download; ms[3] = (double)t.products;
}

int gf2bv_compose_device(const void *d_a, int64_t ra, int64_t a_stride, int64_t n, const void *d_b, int64_t b_stride, int64_t nb,
                         void *d_out, int64_t out_stride, int device, void *stream)
{
	return catching([&]() -> int {
	if (!d_a || !d_b || !d_out) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_compose(ra, n, nb);
	if (!rc) rc = check_device_rows(d_a, a_stride, form_words(n), "d_a needs 16-byte alignment and an even a_stride covering n + 1 bits");
	if (!rc) rc = check_device_rows(d_b, b_stride, form_words(nb), "d_b needs 16-byte alignment and an even b_stride covering nb + 1 bits");
	if (!rc) rc = check_device_rows(d_out, out_stride, form_words(nb), "d_out needs 16-byte alignment and an even out_stride covering nb + 1 bits");
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	g_compose_times = ComposeTimes();
	return enqueue_compose((const u64 *)d_a, ra, a_stride, n, (const u64 *)d_b, b_stride, nb, (u64 *)d_out, out_stride, (hipStream_t)stream);
	});
}

int gf2bv_compose_words(const uint64_t *a, int64_t ra, int64_t a_stride, int64_t n, const uint64_t *b, int64_t b_stride, int64_t nb,
                        uint64_t *out, int64_t out_stride, int device)
{
	return catching([&]() -> int {
	if (!a || !b || !out) return fail(GF2BV_ERR_ARG, "null pointer");
	int rc = check_compose(ra, n, nb);
	if (rc) return rc;
	const i64 wa = form_words(n), wb = form_words(nb);
	if (a_stride < wa) return fail(GF2BV_ERR_ARG, "a_stride does not cover n + 1 bits");
	if (b_stride < wb || out_stride < wb) return fail(GF2BV_ERR_ARG, "b_stride or out_stride does not cover nb + 1 bits");
	if ((rc = check_device(device))) return rc;
	g_compose_times = ComposeTimes();
	if (ra == 0) return GF2BV_OK;
	const i64 das = round_up(wa, 2), dbs = round_up(wb, 2);
	ComposeStage sg(device);
	u64 *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
	if ((rc = sg.open(nullptr, true))) return rc;
	if ((rc = sg.alloc(&d_a, ra * das)) || (rc = sg.alloc(&d_b, n * dbs)) || (rc = sg.alloc(&d_out, ra * dbs))) return rc;
	if ((rc = sg.mark(0))) return rc;
	if ((rc = copy_rows(d_a, das, a, a_stride, wa, ra, hipMemcpyHostToDevice, sg.held.st))) return rc;
	if ((rc = copy_rows(d_b, dbs, b, b_stride, wb, n, hipMemcpyHostToDevice, sg.held.st))) return rc;
	if ((rc = sg.mark(1))) return rc;
	if ((rc = enqueue_compose(d_a, ra, das, n, d_b, dbs, nb, d_out, dbs, sg.held.st))) return rc;
	if ((rc = sg.mark(2))) return rc;
	if ((rc = copy_rows(out, out_stride, d_out, dbs, wb, ra, hipMemcpyDeviceToHost, sg.held.st))) return rc;
	if ((rc = sg.mark(3))) return rc;
	HIPCHK(hipStreamSynchronize(sg.held.st));
	if (out_stride > wb)
		for (i64 r = 0; r < ra; r++) memset(out + r * out_stride + wb, 0, sizeof(u64) * (size_t)(out_stride - wb));
	return sg.times();
	});
}

int gf2bv_compose_power_device(const void *d_b, int64_t b_stride, int64_t n, const uint64_t *k_words, int64_t k_nwords, void *d_out,
                               int64_t out_stride, int device, void *stream)
{
	return catching([&]() -> int {
	int rc = check_power(d_b, b_stride, n, k_words, k_nwords, d_out, out_stride);
	if (!rc) rc = check_device_rows(d_b, b_stride, form_words(n), "d_b needs 16-byte alignment and an even b_stride covering n + 1 bits");
	if (!rc) rc = check_device_rows(d_out, out_stride, form_words(n), "d_out needs 16-byte alignment and an even out_stride covering n + 1 bits");
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	g_compose_times = ComposeTimes();
	const i64 ws = round_up(form_words(n), 2);
	ComposeStage sg(device);
	u64 *base = nullptr, *cur = nullptr, *tmp = nullptr;
	if ((rc = sg.open((hipStream_t)stream, false))) return rc;
	if ((rc = sg.alloc(&base, (n + 1) * ws)) || (rc = sg.alloc(&cur, (n + 1) * ws)) || (rc = sg.alloc(&tmp, (n + 1) * ws))) return rc;
	for (int i = 0; i < 2; i++) if ((rc = sg.mark(i))) return rc;
	// (the map is copied: d_out may be d_b, and the caller's rows are not read after the copy)
	if ((rc = copy_rows(base + ws, ws, d_b, b_stride, form_words(n), n, hipMemcpyDeviceToDevice, sg.held.st))) return rc;
	if ((rc = enqueue_power(base + ws, ws, n, k_words, k_nwords, cur, tmp, ws, (u64 *)d_out, out_stride, sg.held.st))) return rc;
	for (int i = 2; i < 4; i++) if ((rc = sg.mark(i))) return rc;
	HIPCHK(hipStreamSynchronize(sg.held.st));           // the three buffers go back to the pool: the host waits
	return sg.times();
	});
}

int gf2bv_compose_power_words(const uint64_t *b, int64_t b_stride, int64_t n, const uint64_t *k_words, int64_t k_nwords, uint64_t *out,
                              int64_t out_stride, int device)
{
	return catching([&]() -> int {
	int rc = check_power(b, b_stride, n, k_words, k_nwords, out, out_stride);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	g_compose_times = ComposeTimes();
	const i64 w = form_words(n), ws = round_up(w, 2);
	ComposeStage sg(device);
	u64 *base = nullptr, *cur = nullptr, *tmp = nullptr;
	const u64 *d_out = nullptr;
	if ((rc = sg.open(nullptr, true))) return rc;
	if ((rc = sg.alloc(&base, (n + 1) * ws)) || (rc = sg.alloc(&cur, (n + 1) * ws)) || (rc = sg.alloc(&tmp, (n + 1) * ws))) return rc;
	if ((rc = sg.mark(0))) return rc;
	if ((rc = copy_rows(base + ws, ws, b, b_stride, w, n, hipMemcpyHostToDevice, sg.held.st))) return rc;
	if ((rc = sg.mark(1))) return rc;
	if ((rc = enqueue_power(base + ws, ws, n, k_words, k_nwords, cur, tmp, ws, nullptr, 0, sg.held.st, &d_out))) return rc;
	if ((rc = sg.mark(2))) return rc;
	if ((rc = copy_rows(out, out_stride, d_out, ws, w, n, hipMemcpyDeviceToHost, sg.held.st))) return rc;
	if ((rc = sg.mark(3))) return rc;
	HIPCHK(hipStreamSynchronize(sg.held.st));
	if (out_stride > w)
		for (i64 r = 0; r < n; r++) memset(out + r * out_stride + w, 0, sizeof(u64) * (size_t)(out_stride - w));
	return sg.times();
	});
}

int gf2bv_compose_unroll_device(const void *d_a, int64_t ra, int64_t a_stride, int64_t n, const void *d_b, int64_t b_stride,
                                const uint64_t *start_words, int64_t start_nwords, const uint64_t *step_words, int64_t step_nwords,
                                int64_t count, void *d_out, int64_t out_stride, int device, void *stream)
{
	return catching([&]() -> int {
	int rc = check_unroll(d_a, ra, a_stride, n, d_b, b_stride, start_words, start_nwords, step_words, step_nwords, count, d_out, out_stride);
	if (!rc) rc = check_device_rows(d_a, a_stride, form_words(n), "d_a needs 16-byte alignment and an even a_stride covering n + 1 bits");
	if (!rc) rc = check_device_rows(d_b, b_stride, form_words(n), "d_b needs 16-byte alignment and an even b_stride covering n + 1 bits");
	if (!rc) rc = check_device_rows(d_out, out_stride, form_words(n), "d_out needs 16-byte alignment and an even out_stride covering n + 1 bits");
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	g_compose_times = ComposeTimes();
	if (ra == 0 || count == 0) return GF2BV_OK;
	const i64 ws = round_up(form_words(n), 2);
	ComposeStage sg(device);
	u64 *base = nullptr, *cur = nullptr, *tmp = nullptr;
	if ((rc = sg.open((hipStream_t)stream, false))) return rc;
	if ((rc = sg.alloc(&base, (n + 1) * ws)) || (rc = sg.alloc(&cur, (n + 1) * ws)) || (rc = sg.alloc(&tmp, (n + 1) * ws))) return rc;
	for (int i = 0; i < 2; i++) if ((rc = sg.mark(i))) return rc;
	// (the map is copied before anything else: the caller's rows are not read after the copy)
	if ((rc = copy_rows(base + ws, ws, d_b, b_stride, form_words(n), n, hipMemcpyDeviceToDevice, sg.held.st))) return rc;
	if ((rc = enqueue_unroll((const u64 *)d_a, ra, a_stride, n, base, cur, tmp, ws, start_words, start_nwords, step_words, step_nwords, count,
	                         (u64 *)d_out, out_stride, sg.held.st))) return rc;
	for (int i = 2; i < 4; i++) if ((rc = sg.mark(i))) return rc;
	HIPCHK(hipStreamSynchronize(sg.held.st));           // the three buffers go back to the pool: the host waits
	return sg.times();
	});
}

int gf2bv_compose_unroll_words(const uint64_t *a, int64_t ra, int64_t a_stride, int64_t n, const uint64_t *b, int64_t b_stride,
                               const uint64_t *start_words, int64_t start_nwords, const uint64_t *step_words, int64_t step_nwords,
                               int64_t count, uint64_t *out, int64_t out_stride, int device)
{
	return catching([&]() -> int {
	int rc = check_unroll(a, ra, a_stride, n, b, b_stride, start_words, start_nwords, step_words, step_nwords, count, out, out_stride);
	if (!rc) rc = check_device(device);
	if (rc) return rc;
	g_compose_times = ComposeTimes();
	if (ra == 0 || count == 0) return GF2BV_OK;
	const i64 w = form_words(n), ws = round_up(w, 2), rows = count * ra;
	ComposeStage sg(device);
	u64 *base = nullptr, *cur = nullptr, *tmp = nullptr, *d_a = nullptr, *d_out = nullptr;
	if ((rc = sg.open(nullptr, true))) return rc;
	if ((rc = sg.alloc(&base, (n + 1) * ws)) || (rc = sg.alloc(&cur, (n + 1) * ws)) || (rc = sg.alloc(&tmp, (n + 1) * ws))) return rc;
	if ((rc = sg.alloc(&d_a, ra * ws)) || (rc = sg.alloc(&d_out, rows * ws))) return rc;
	if ((rc = sg.mark(0))) return rc;
	if ((rc = copy_rows(base + ws, ws, b, b_stride, w, n, hipMemcpyHostToDevice, sg.held.st))) return rc;
	if ((rc = copy_rows(d_a, ws, a, a_stride, w, ra, hipMemcpyHostToDevice, sg.held.st))) return rc;
	if ((rc = sg.mark(1))) return rc;
	if ((rc = enqueue_unroll(d_a, ra, ws, n, base, cur, tmp, ws, start_words, start_nwords, step_words, step_nwords, count, d_out, ws, sg.held.st))) return rc;
	if ((rc = sg.mark(2))) return rc;
	if ((rc = copy_rows(out, out_stride, d_out, ws, w, rows, hipMemcpyDeviceToHost, sg.held.st))) return rc;
	if ((rc = sg.mark(3))) return rc;
	HIPCHK(hipStreamSynchronize(sg.held.st));
	if (out_stride > w)
		for (i64 r = 0; r < rows; r++) memset(out + r * out_stride + w, 0, sizeof(u64) * (size_t)(out_stride - w));
	return sg.times();
	});
}

}  // extern "C"
