// Probe for "one T per block": the block TRSM as it is (k_block_trsm: a chain of four dependent stages, 8 table builds, 16 barriers)
// against the same pivot rows formed in ONE table pass as P = T x S_raw, where T -- the 256-bit selection over the block's 4 x 64
// source slots behind every final pivot row -- is what the chain leaves when it runs on the identity.  T depends on the block's
// records alone, so a solve could make it once per block; here it is made by running k_block_trsm itself on an identity matrix.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe_block_t.hip -o /tmp/probe_block_t && /tmp/probe_block_t [groups]
// Synthetic records (random combinations and multipliers, a random row permutation, one panel with 40 pivots), a resident matrix
// of `groups` 4-word groups (default 128 = the trailing 256 tiles of a 65536^2 solve's mid-range); both kernels' in-place rows and
// compact Pc output compared word for word, then timed: launches back to back, and one at a time with a synchronise between.
// The look-ahead (k_prio_window) is probed by a copy of its compute part -- every workgroup forms the pivot rows on the next
// window's four words and folds them into its 256 rows, whose tables of the FINAL pivot rows it needs either way -- with the chain as
// it is and with P = T x S in front of the four table builds; `rows / 256` workgroups, window words and pivot rows compared.
#define GF2_TW 2
#include "../gf2bv_amd/csrc/gf2_kernels.hip.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

static u64 rng_state = 88172645463325252ull;
static u64 rnd() { u64 &x = rng_state; x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }

// T[g][pivot bit][4 words]: bit s of word h = source slot s of panel h takes part in that pivot row
__global__ void __launch_bounds__(256)
k_block_trsm_T(u64 *__restrict__ M, i64 srows, int j0, int gb, int wlo, int group_begin,
               const PanelRec *__restrict__ panels, const PanelAux *__restrict__ aux, const u64 *__restrict__ T,
               int nw_lo, int nw_hi, u64 *__restrict__ Pc)
{
	constexpr int WPW = 4;
	__shared__ u64 S[GF2_GMAX * 64 * WPW];        // raw source rows, [panel][slot][word]
	__shared__ u64 Tn[32 * 16 * WPW];             // nibble tables of 128 source rows
	const i64 w0 = (i64)(blockIdx.x + group_begin) * WPW;
	const int t = threadIdx.x, r = t / WPW, w = t % WPW;
	auto at = [&](i64 row) -> u64 & { return M[tidx(row, w0 + w, srows)]; };
	const bool live = w0 + w >= wlo && !(w0 + w >= nw_lo && w0 + w < nw_hi);
	PanelRec rec[GF2_GMAX];
	int srow[GF2_GMAX];
	u64 Tr[GF2_GMAX][4];
#pragma unroll
	for (int g = 0; g < GF2_GMAX; g++) {
		const int gc = g < gb ? g : 0;
		rec[g] = panels[j0 + gc];
		srow[g] = aux[j0 + gc].slot_row[r];
		const ulonglong4 tv = *reinterpret_cast<const ulonglong4 *>(T + (g * 64 + r) * 4);
		Tr[g][0] = tv.x; Tr[g][1] = tv.y; Tr[g][2] = tv.z; Tr[g][3] = tv.w;
		if (g >= gb) { rec[g].p = 0; rec[g].mask = 0; Tr[g][0] = Tr[g][1] = Tr[g][2] = Tr[g][3] = 0; }
	}
	int prow[GF2_GMAX];                            // where pivot BIT r of panel g is stored in place (-1: no such pivot)
#pragma unroll
	for (int g = 0; g < GF2_GMAX; g++) {
		const bool has = (rec[g].mask >> r) & 1;
		const int k = __popcll(rec[g].mask & lanemask_lt(r));
		const int pr = aux[j0 + (g < gb ? g : 0)].slot_row[has ? k : 0];
		prow[g] = has ? pr : -1;
		const u64 v = at(r < rec[g].p ? srow[g] : 0);
		S[(g * 64 + r) * WPW + w] = (r < rec[g].p && live) ? v : 0ull;
	}
	__syncthreads();
	auto build_tables = [&](const u64 *rows64, int n) {      // nibble n of rows64: 16 entries x 4 words, one entry per thread
		const int v = t & 15;
		u64 a[WPW] = { 0, 0, 0, 0 };
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const u64 on = ((v >> k) & 1) ? ~0ull : 0ull;
#pragma unroll
			for (int e = 0; e < WPW; e++) a[e] ^= rows64[(4 * n + k) * WPW + e] & on;
		}
#pragma unroll
		for (int e = 0; e < WPW; e++) Tn[(n * 16 + v) * WPW + e] = a[e];
	};
	u64 acc[GF2_GMAX] = { 0, 0, 0, 0 };
#pragma unroll
	for (int half = 0; half < 2; half++) {
		if (half) __syncthreads();
		build_tables(&S[half * 128 * WPW], t >> 4);
		build_tables(&S[half * 128 * WPW], 16 + (t >> 4));
		__syncthreads();
#pragma unroll
		for (int g = 0; g < GF2_GMAX; g++)
#pragma unroll
			for (int n = 0; n < 32; n++) {
				const u64 sel = Tr[g][half * 2 + (n >> 4)];
				acc[g] ^= Tn[(n * 16 + (int)((sel >> (4 * (n & 15))) & 15)) * WPW + w];
			}
	}
	const i64 wabs = w0 + w;
#pragma unroll
	for (int g = 0; g < GF2_GMAX; g++) {
		if (prow[g] >= 0 && live) at(prow[g]) = acc[g];
		if (Pc) Pc[(((wabs >> 1) * GF2_GMAX + g) * 64 + r) * 2 + (wabs & 1)] = acc[g];
	}
}

// k_prio_window's compute part (steps (i) and (ii) of its comment) on the four words from wlo on; mplain[g * rows + row]: the row's
// multiplier for panel g in plain bit order.  WITH_T: the pivot rows come as T x S_raw, then one table build per panel for the rows.
template <bool WITH_T>
__global__ void __launch_bounds__(256)
k_lookahead_probe(const u64 *__restrict__ M, i64 rows, i64 srows, int j0, int gb, int wlo,
                  const PanelRec *__restrict__ panels, const PanelAux *__restrict__ aux, const u64 *__restrict__ T,
                  const u64 *__restrict__ mplain, u64 *__restrict__ Wout, u64 *__restrict__ Pout)
{
	constexpr int W = GF2_GMAX;
	__shared__ u64 S[GF2_GMAX * 64 * W];
	u64 *const Pbit = S;
	__shared__ u64 Tn[(WITH_T ? 32 : 16) * 16 * W];
	__shared__ int Bk[GF2_GMAX * 64];
	const int t = threadIdx.x, r = t / W, w = t % W;
	const i64 i = (i64)blockIdx.x * 256 + t, ic = i < rows ? i : rows - 1;
	PanelRec rec[GF2_GMAX];
	int srow[GF2_GMAX];
	u64 comb[GF2_GMAX], smul[GF2_GMAX][GF2_GMAX], mrow[GF2_GMAX], Tr[GF2_GMAX][4];
#pragma unroll
	for (int g = 0; g < GF2_GMAX; g++) {
		const int gc = g < gb ? g : 0;
		rec[g] = panels[j0 + gc];
		srow[g] = aux[j0 + gc].slot_row[r];
		if (WITH_T) {
			const ulonglong4 tv = *reinterpret_cast<const ulonglong4 *>(T + (g * 64 + r) * 4);
			Tr[g][0] = tv.x; Tr[g][1] = tv.y; Tr[g][2] = tv.z; Tr[g][3] = tv.w;
		} else {
			comb[g] = aux[j0 + gc].comb[r];
#pragma unroll
			for (int e = 0; e < GF2_GMAX; e++) smul[g][e] = (e < g) ? aux[j0 + gc].src_mult[r][e] : 0ull;
		}
		mrow[g] = mplain[(i64)gc * rows + ic];
		if (g >= gb) { rec[g].p = 0; rec[g].mask = 0; mrow[g] = 0; }
	}
	u64 wv[W];
#pragma unroll
	for (int e = 0; e < W; e++) wv[e] = M[tidx(ic, wlo + e, srows)];
#pragma unroll
	for (int g = 0; g < GF2_GMAX; g++) {
		const u64 v = M[tidx(r < rec[g].p ? srow[g] : 0, wlo + w, srows)];
		S[(g * 64 + r) * W + w] = r < rec[g].p ? v : 0ull;
		if (!WITH_T && w == 0 && ((rec[g].mask >> r) & 1)) Bk[g * 64 + __popcll(rec[g].mask & lanemask_lt(r))] = r;
	}
	__syncthreads();
	auto build_tables = [&](const u64 *rows64, int n) {
		const int v = t & 15;
		u64 a[W] = { 0, 0, 0, 0 };
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const u64 on = ((v >> k) & 1) ? ~0ull : 0ull;
#pragma unroll
			for (int e = 0; e < W; e++) a[e] ^= rows64[(4 * n + k) * W + e] & on;
		}
#pragma unroll
		for (int e = 0; e < W; e++) Tn[(n * 16 + v) * W + e] = a[e];
	};
	auto rows_take = [&](int g) {
		if (i < rows && mrow[g]) {
			u64 acc[W];
			nibble_rows(Tn, mrow[g], acc);
#pragma unroll
			for (int e = 0; e < W; e++) wv[e] ^= acc[e];
		}
	};
	if (WITH_T) {
		u64 acc[GF2_GMAX] = { 0, 0, 0, 0 };
#pragma unroll
		for (int half = 0; half < 2; half++) {
			if (half) __syncthreads();
			build_tables(&S[half * 128 * W], t >> 4);
			build_tables(&S[half * 128 * W], 16 + (t >> 4));
			__syncthreads();
#pragma unroll
			for (int g = 0; g < GF2_GMAX; g++)
#pragma unroll
				for (int n = 0; n < 32; n++) {
					const u64 sel = Tr[g][half * 2 + (n >> 4)];
					acc[g] ^= Tn[(n * 16 + (int)((sel >> (4 * (n & 15))) & 15)) * W + w];
				}
		}
		__syncthreads();
#pragma unroll
		for (int g = 0; g < GF2_GMAX; g++) Pbit[(g * 64 + r) * W + w] = acc[g];
		__syncthreads();
#pragma unroll
		for (int g = 0; g < GF2_GMAX; g++) {
			if (g >= gb) break;
			build_tables(&Pbit[g * 64 * W], t >> 4);
			__syncthreads();
			rows_take(g);
			__syncthreads();
		}
	} else {
#pragma unroll
		for (int g = 0; g < GF2_GMAX; g++) {
			if (g >= gb) break;
			build_tables(&S[g * 64 * W], t >> 4);
			__syncthreads();
			if (!((rec[g].mask >> r) & 1)) Pbit[(g * 64 + r) * W + w] = 0;
			if (r < rec[g].p) Pbit[(g * 64 + Bk[g * 64 + r]) * W + w] = nibble_word(Tn, comb[g], w);
			__syncthreads();
			build_tables(&Pbit[g * 64 * W], t >> 4);
			__syncthreads();
#pragma unroll
			for (int h = g + 1; h < GF2_GMAX; h++)
				if (h < gb && r < rec[h].p) S[(h * 64 + r) * W + w] ^= nibble_word(Tn, smul[h][g], w);
			rows_take(g);
			__syncthreads();
		}
	}
	if (blockIdx.x == 0)
#pragma unroll
		for (int g = 0; g < GF2_GMAX; g++) Pout[(g * 64 + r) * W + w] = Pbit[(g * 64 + r) * W + w];
	if (i >= rows) return;
#pragma unroll
	for (int e = 0; e < W; e++) Wout[i * GF2_GMAX + e] = wv[e];
}

int main(int argc, char **argv)
{
	const int ng = argc > 1 ? atoi(argv[1]) : 128;
	const i64 srows = 512, tiles = 2 * (i64)ng;
	const size_t mwords = (size_t)tiles * srows * 2, pcwords = (size_t)tiles * GF2_GMAX * 64 * 2;
	// records
	std::vector<PanelRec> hp(GF2_GMAX); std::vector<PanelAux> ha(GF2_GMAX);
	std::vector<int> perm(256);
	for (int i = 0; i < 256; i++) perm[i] = i;
	for (int i = 255; i > 0; i--) std::swap(perm[i], perm[rnd() % (i + 1)]);
	int start = 0;
	for (int g = 0; g < GF2_GMAX; g++) {
		memset(&ha[g], 0, sizeof(PanelAux));
		u64 mask = ~0ull;
		if (g == 2) { mask = 0; while (__builtin_popcountll(mask) < 40) mask |= 1ull << (rnd() & 63); }
		hp[g].start = start; hp[g].p = __builtin_popcountll(mask); hp[g].mask = mask;
		start += hp[g].p;
		for (int k = 0; k < 64; k++) {
			ha[g].slot_row[k] = perm[g * 64 + k];
			ha[g].comb[k] = k < hp[g].p ? rnd() : 0;
			for (int e = 0; e < GF2_GMAX; e++) ha[g].src_mult[k][e] = (e < g && k < hp[g].p) ? rnd() : 0;
		}
		// (sources and combinations of a short panel use its first p slots only, as the search leaves them)
		if (hp[g].p < 64) for (int k = 0; k < 64; k++) ha[g].comb[k] &= (1ull << hp[g].p) - 1;
	}
	PanelRec *panels; PanelAux *aux;
	CK(hipMalloc(&panels, sizeof(PanelRec) * GF2_GMAX)); CK(hipMemcpy(panels, hp.data(), sizeof(PanelRec) * GF2_GMAX, hipMemcpyHostToDevice));
	CK(hipMalloc(&aux, sizeof(PanelAux) * GF2_GMAX)); CK(hipMemcpy(aux, ha.data(), sizeof(PanelAux) * GF2_GMAX, hipMemcpyHostToDevice));
	const SysStride ss{0, 0};
	// T = the chain on the identity: one group whose source row (g, r) is bit r of word g
	u64 *MI, *PcI, *T;
	{
		std::vector<u64> hi((size_t)2 * srows * 2, 0);
		for (int g = 0; g < GF2_GMAX; g++)
			for (int r = 0; r < hp[g].p; r++) hi[((size_t)(g >> 1) * srows + ha[g].slot_row[r]) * 2 + (g & 1)] = 1ull << r;
		CK(hipMalloc(&MI, hi.size() * 8)); CK(hipMemcpy(MI, hi.data(), hi.size() * 8, hipMemcpyHostToDevice));
		CK(hipMalloc(&PcI, (size_t)2 * GF2_GMAX * 64 * 2 * 8));
		k_block_trsm<2, 4><<<dim3(1, 1), dim3(256), 0>>>(MI, srows, 0, GF2_GMAX, 0, 0, 1, 0, panels, aux, 0, 0, PcI, ss);
		CK(hipDeviceSynchronize());
		std::vector<u64> hpc((size_t)2 * GF2_GMAX * 64 * 2), ht((size_t)GF2_GMAX * 64 * 4);
		CK(hipMemcpy(hpc.data(), PcI, hpc.size() * 8, hipMemcpyDeviceToHost));
		for (int g = 0; g < GF2_GMAX; g++)
			for (int b = 0; b < 64; b++)
				for (int w = 0; w < 4; w++) ht[((size_t)g * 64 + b) * 4 + w] = hpc[((((size_t)(w >> 1)) * GF2_GMAX + g) * 64 + b) * 2 + (w & 1)];
		CK(hipMalloc(&T, ht.size() * 8)); CK(hipMemcpy(T, ht.data(), ht.size() * 8, hipMemcpyHostToDevice));
	}
	// the same random matrix through both
	std::vector<u64> h0(mwords), hA(mwords), hB(mwords), pA(pcwords), pB(pcwords);
	for (auto &v : h0) v = rnd();
	u64 *M, *Pc;
	CK(hipMalloc(&M, mwords * 8)); CK(hipMalloc(&Pc, pcwords * 8));
	CK(hipMemcpy(M, h0.data(), mwords * 8, hipMemcpyHostToDevice)); CK(hipMemset(Pc, 0xff, pcwords * 8));
	k_block_trsm<2, 4><<<dim3(ng, 1), dim3(256), 0>>>(M, srows, 0, GF2_GMAX, 0, 0, 1, 0, panels, aux, 0, 0, Pc, ss);
	CK(hipDeviceSynchronize());
	CK(hipMemcpy(hA.data(), M, mwords * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(pA.data(), Pc, pcwords * 8, hipMemcpyDeviceToHost));
	CK(hipMemcpy(M, h0.data(), mwords * 8, hipMemcpyHostToDevice)); CK(hipMemset(Pc, 0xff, pcwords * 8));
	k_block_trsm_T<<<dim3(ng), dim3(256), 0>>>(M, srows, 0, GF2_GMAX, 0, 0, panels, aux, T, 0, 0, Pc);
	CK(hipDeviceSynchronize());
	CK(hipMemcpy(hB.data(), M, mwords * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(pB.data(), Pc, pcwords * 8, hipMemcpyDeviceToHost));
	size_t badm = 0, badp = 0, changed = 0;
	for (size_t i = 0; i < mwords; i++) { badm += hA[i] != hB[i]; changed += hA[i] != h0[i]; }
	for (size_t i = 0; i < pcwords; i++) badp += pA[i] != pB[i];
	printf("P = T x S against the chain, %d groups: %zu matrix words changed by the chain, %zu differ; Pc: %zu of %zu words differ\n", ng, changed, badm, badp, pcwords);
	if (badm || badp) return 1;
	// time
	hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
	const int reps = 200;
	auto chain = [&] { k_block_trsm<2, 4><<<dim3(ng, 1), dim3(256), 0>>>(M, srows, 0, GF2_GMAX, 0, 0, 1, 0, panels, aux, 0, 0, Pc, ss); };
	auto withT = [&] { k_block_trsm_T<<<dim3(ng), dim3(256), 0>>>(M, srows, 0, GF2_GMAX, 0, 0, panels, aux, T, 0, 0, Pc); };
	for (int round = 0; round < 3; round++)
		for (int which = 0; which < 2; which++) {
			for (int i = 0; i < 10; i++) { if (which) withT(); else chain(); }
			CK(hipDeviceSynchronize());
			CK(hipEventRecord(e0));
			for (int i = 0; i < reps; i++) { if (which) withT(); else chain(); }
			CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
			float ms; CK(hipEventElapsedTime(&ms, e0, e1));
			const auto t0 = std::chrono::steady_clock::now();
			for (int i = 0; i < reps; i++) { if (which) withT(); else chain(); CK(hipDeviceSynchronize()); }
			const double one = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
			printf("%s: %.2f us per launch back to back, %.2f us launch + synchronise\n", which ? "P = T x S  " : "chain      ", 1e3 * ms / reps, one);
		}
	// the look-ahead: rows x 4 window words (the first group), plain multipliers (zero for the block's own source rows)
	for (i64 rows : { (i64)65536, (i64)32768 }) {
		const i64 lsr = rows + 64;
		std::vector<u64> hm((size_t)2 * lsr * 2), hmul((size_t)GF2_GMAX * rows);
		for (auto &v : hm) v = rnd();
		for (auto &v : hmul) v = rnd();
		for (int g = 0; g < GF2_GMAX; g++) for (int k = 0; k < 256; k++) hmul[(size_t)g * rows + k] = 0;
		u64 *LM, *mul, *Wo[2], *Po[2];
		CK(hipMalloc(&LM, hm.size() * 8)); CK(hipMemcpy(LM, hm.data(), hm.size() * 8, hipMemcpyHostToDevice));
		CK(hipMalloc(&mul, hmul.size() * 8)); CK(hipMemcpy(mul, hmul.data(), hmul.size() * 8, hipMemcpyHostToDevice));
		for (int k = 0; k < 2; k++) { CK(hipMalloc(&Wo[k], (size_t)rows * 4 * 8)); CK(hipMalloc(&Po[k], 256 * 4 * 8)); }
		const unsigned wgs = (unsigned)((rows + 255) / 256);
		auto la = [&](int which) {
			if (which) k_lookahead_probe<true><<<dim3(wgs), dim3(256), 0>>>(LM, rows, lsr, 0, GF2_GMAX, 0, panels, aux, T, mul, Wo[1], Po[1]);
			else k_lookahead_probe<false><<<dim3(wgs), dim3(256), 0>>>(LM, rows, lsr, 0, GF2_GMAX, 0, panels, aux, T, mul, Wo[0], Po[0]);
		};
		la(0); la(1); CK(hipDeviceSynchronize());
		std::vector<u64> w0((size_t)rows * 4), w1(w0.size()), p0(1024), p1(1024);
		CK(hipMemcpy(w0.data(), Wo[0], w0.size() * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(w1.data(), Wo[1], w1.size() * 8, hipMemcpyDeviceToHost));
		CK(hipMemcpy(p0.data(), Po[0], 8192, hipMemcpyDeviceToHost)); CK(hipMemcpy(p1.data(), Po[1], 8192, hipMemcpyDeviceToHost));
		size_t bw = 0, bp = 0, moved = 0;
		for (size_t k = 0; k < w0.size(); k++) bw += w0[k] != w1[k];
		for (size_t k = 0; k < (size_t)rows; k++) for (int e = 0; e < 4; e++) moved += w0[k * 4 + e] != hm[((size_t)(e >> 1) * lsr + k) * 2 + (e & 1)];
		for (int k = 0; k < 1024; k++) bp += p0[k] != p1[k];
		printf("look-ahead, %lld rows (%u workgroups): %zu window words changed by the chain form, %zu differ; pivot rows by bit: %zu of 1024 words differ\n", (long long)rows, wgs, moved, bw, bp);
		if (bw || bp) return 1;
		for (int round = 0; round < 3; round++)
			for (int which = 0; which < 2; which++) {
				for (int k = 0; k < 10; k++) la(which);
				CK(hipDeviceSynchronize());
				CK(hipEventRecord(e0));
				for (int k = 0; k < reps; k++) la(which);
				CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
				float ms; CK(hipEventElapsedTime(&ms, e0, e1));
				printf("look-ahead %s: %.2f us per launch back to back\n", which ? "P = T x S  " : "chain      ", 1e3 * ms / reps);
			}
		CK(hipFree(LM)); CK(hipFree(mul)); for (int k = 0; k < 2; k++) { CK(hipFree(Wo[k])); CK(hipFree(Po[k])); }
	}
	return 0;
}
