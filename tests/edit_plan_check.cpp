// Brute-force check of csrc/rb2_edit_plan.h, the arithmetic of rb2_hip_approx_ed that needs no GPU: the packed column against a full
// Levenshtein column, a word-trie search driven by the header's functions against the definition of a match over all substrings of tiny
// sets of strings (with the piece bound and without it), the bound against the matches below a node, and the rows, stacks and launches of
// a call (stack_rows, stack_len_cap and stack_passes of csrc/rb2_query_plan.h with this search's row size).  Built and run by tests/test_edit_plan.py, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer; prints
// "EDIT PLAN OK" and leaves with 0 when every property holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "rb2_edit_plan.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static const int INF = 1000;

// ---- the definition, stated once more and in full: sub, lev, ed (include/rb2_hip.h) ----
static int sub(int a, int c) { return (a == c && c >= 1 && c <= 4) ? 0 : 1; }
static int lev(const std::string &X, const std::string &Y)          // X: a word over A C G T; Y: a part of the query
{
	std::vector<std::vector<int>> D(X.size() + 1, std::vector<int>(Y.size() + 1, 0));
	for (size_t i = 0; i <= X.size(); ++i)
		for (size_t j = 0; j <= Y.size(); ++j) {
			if (i == 0 || j == 0) { D[i][j] = (int)(i + j); continue; }
			D[i][j] = std::min(std::min(D[i - 1][j] + 1, D[i][j - 1] + 1), D[i - 1][j - 1] + sub(X[i - 1], Y[j - 1]));
		}
	return D[X.size()][Y.size()];
}
static int ed(const std::string &S, const std::string &q)
{
	if (q.size() >= 2 && S.size() >= 2) return sub(S[0], q[0]) + lev(S.substr(1, S.size() - 2), q.substr(1, q.size() - 2)) + sub(S.back(), q.back());
	if (q.size() == 1 && S.size() == 1) return sub(S[0], q[0]);
	return INF;
}

// ---- rows, stacks and passes ----
static long check_launches()
{
	long n = 0, two = 0;
	CHECK(edit_row_bytes(1, 0) == 72 + 8 + 8 && edit_row_bytes(8, 0) == 72 * 8 + 16 && edit_row_bytes(8, 4) == 72 * 12 + 16 + 8 && edit_nodes(40, 2) == 42, "row bytes");
	const int64_t sizes[] = {1, 87, 88, 89, 4096, 65536, 74 * 8192, 16 * 75 * 8192, (int64_t)1 << 24, APPROX_SCRATCH_BYTES};
	const int64_t ns[] = {1, 2, 15, 16, 17, 300, 440, 441, 16383, 16384, 16385, 40000, 1 << 20, (int64_t)1 << 24};
	const int64_t lens[] = {1, 2, 7, 8, 9, 40, 101, 216, 217, 221, 222, 1000, 8191, 8192};
	for (int E = 0; E <= EDIT_MAX_ED; ++E) {
		const auto rb_of = [E](int64_t L) { return edit_row_bytes(L, E); };
		for (int64_t L = 1; L <= APPROX_MAX_LEN; ++L) {
			const int64_t rb = edit_row_bytes(L, E), P = edit_nodes(L, E);
			CHECK(rb % 8 == 0 && rb >= 64 * P + 8 * P + P + L && rb < 73 * P + L + 16, "L %lld", (long long)L);
			CHECK(P >= L - 1 + E + 1, "the root and L - 1 + max_ed nodes");
			CHECK(L == 1 || rb > edit_row_bytes(L - 1, E), "L %lld", (long long)L);
		}
		for (int64_t bytes : sizes) {
			for (int64_t rows : {(int64_t)1, (int64_t)16, (int64_t)440, APPROX_SHORT_ROWS, APPROX_ROWS}) {
				const int64_t c = stack_len_cap(rows, bytes, rb_of);
				CHECK(c >= 0 && c <= APPROX_MAX_LEN, "cap");
				CHECK(c == 0 || edit_row_bytes(c, E) * rows <= bytes, "rows %lld bytes %lld: cap %lld does not fit", (long long)rows, (long long)bytes, (long long)c);
				CHECK(c == APPROX_MAX_LEN || edit_row_bytes(c + 1, E) * rows > bytes, "rows %lld bytes %lld: cap %lld could be larger", (long long)rows, (long long)bytes, (long long)c);
				++n;
			}
			for (int64_t nq : ns)
				for (int64_t lmax : lens) {
					const int64_t r = stack_rows(nq, edit_row_bytes(lmax, E), bytes, APPROX_ROWS);
					CHECK(r >= 1 && r <= nq && r <= APPROX_ROWS, "rows");
					CHECK(r == 1 || r * edit_row_bytes(lmax, E) <= bytes, "n %lld L %lld bytes %lld: %lld rows do not fit", (long long)nq, (long long)lmax, (long long)bytes, (long long)r);
					CHECK(r == nq || r == APPROX_ROWS || (r + 1) * edit_row_bytes(lmax, E) > bytes, "n %lld L %lld bytes %lld: %lld rows could be more", (long long)nq, (long long)lmax, (long long)bytes, (long long)r);
					int64_t pass[2][4];
					const int np = stack_passes(nq, lmax, bytes, rb_of, pass);
					CHECK(np == 1 || np == 2, "passes");
					two += np == 2;
					for (int k = 0; k < np; ++k) {
						CHECK(pass[k][3] >= 1 && pass[k][3] <= nq && pass[k][3] <= APPROX_ROWS && pass[k][2] >= 1 && pass[k][2] <= lmax, "pass %d", k);
						CHECK(pass[k][3] == 1 || pass[k][3] * edit_row_bytes(pass[k][2], E) <= bytes, "pass %d: the stacks do not fit the scratch", k);
					}
					const int64_t probe[] = {INT64_MIN, -5, -1, 0, 1, 2, 8, 9, 216, 217, 221, 222, lmax - 1, lmax, lmax + 1, APPROX_MAX_LEN, APPROX_MAX_LEN + 1, INT64_MAX};
					for (int64_t L : probe) {                           // what k_approx_ed asks: lmin < L <= lcap
						int owners = 0;
						for (int k = 0; k < np; ++k)
							if (L > pass[k][0] && L <= pass[k][1]) {
								++owners;
								CHECK(L > lmax || L <= pass[k][2], "n %lld lmax %lld bytes %lld: a query of %lld in a launch with stacks for %lld", (long long)nq, (long long)lmax, (long long)bytes, (long long)L, (long long)pass[k][2]);
							}
						CHECK(owners == 1 || (L == INT64_MIN && owners == 0), "n %lld lmax %lld bytes %lld: length %lld has %d launches", (long long)nq, (long long)lmax, (long long)bytes, (long long)L, owners);
					}
					if (np == 2) CHECK(pass[0][3] > pass[1][3] && pass[0][2] < pass[1][2], "the short launch must have more rows");
					++n;
				}
		}
	}
	int64_t pass[2][4];
	const auto rb2 = [](int64_t L) { return edit_row_bytes(L, 2); };
	CHECK(stack_passes(100000, APPROX_MAX_LEN, APPROX_SCRATCH_BYTES, rb2, pass) == 2 && pass[0][1] == stack_len_cap(APPROX_SHORT_ROWS, APPROX_SCRATCH_BYTES, rb2) && pass[0][1] > 200 && pass[0][1] < 222 &&
	      pass[0][3] >= APPROX_SHORT_ROWS && pass[1][3] >= 440 && pass[1][3] <= 443, "the _dev variant: %lld %lld %lld", (long long)pass[0][1], (long long)pass[0][3], (long long)pass[1][3]);
	CHECK(stack_passes(100000, 101, APPROX_SCRATCH_BYTES, rb2, pass) == 1 && pass[0][3] == APPROX_ROWS, "reads of 101");
	CHECK(stack_passes(400, APPROX_MAX_LEN, APPROX_SCRATCH_BYTES, [](int64_t L) { return edit_row_bytes(L, 4); }, pass) == 1 && pass[0][3] == 400, "few queries");
	CHECK(two > 0, "no case had two launches");
	return n;
}

// ---- the packed column against the full one: every depth, every field ----
static long check_columns()
{
	long n = 0, small = 0, capped = 0, none = 0;
	for (int t = 0; t < 4000; ++t) {
		const int L = 2 + (int)(rnd() % 11), M = L - 2, E = (int)(rnd() % (EDIT_MAX_ED + 1)), cap = E + 1;
		uint8_t q[16];
		std::string tq;
		for (int i = 0; i < L; ++i) q[i] = (uint8_t)(rnd() % 7 == 0 ? 5 : 1 + rnd() % 4);
		for (int i = 1; i < L - 1; ++i) tq.push_back((char)q[i]);
		std::string W;                                         // W': grows at its front
		uint64_t col = edit_init(M, cap);
		for (int d = 0; d <= M + EDIT_MAX_ED + 2; ++d) {
			if (d > 0) {
				int a = 1 + (int)(rnd() % 4);                      // mostly the symbol of the query, so that small cells stay
				if (d <= M && rnd() % 4 && q[L - 1 - d] != 5) a = q[L - 1 - d];
				W.insert(W.begin(), (char)a);
				col = edit_step(col, edit_window(q, M, d), a, cap);
			}
			const uint64_t win = edit_window(q, M, d), needs = edit_needs(nullptr, 0, M, d);
			int best = INF;
			for (int b = 0; b < EDIT_CELLS; ++b) {
				const int64_t j = edit_j(M, d, b);
				const int v = edit_cell(col, b);
				if (j < 0 || j > M) {
					CHECK(v == cap && edit_cell(win, b) == EDIT_NONE && edit_cell(needs, b) == EDIT_NONE, "L %d d %d field %d: a field without a cell holds %d", L, d, b, v);
					++none;
					continue;
				}
				const int want = lev(W, tq.substr((size_t)j));
				CHECK(v == std::min(want, cap), "L %d max_ed %d depth %d cell %lld: packed %d, full %d", L, E, d, (long long)j, v, want);
				CHECK(edit_cell(win, b) == (j == M ? 0 : q[j + 1]) && edit_cell(needs, b) == 0, "window");
				small += want <= E; capped += want > E;
				best = std::min(best, want);
			}
			for (int j = 0; j <= M; ++j) {                         // outside the band no cell is small: the band loses nothing
				const int want = lev(W, tq.substr((size_t)j));
				if (std::abs(j - (M - d)) > EDIT_MAX_ED) CHECK(want > EDIT_MAX_ED, "a cell outside the band holds %d", want);
				if (std::abs(j - (M - d)) > E) CHECK(want > E, "a cell outside the band of max_ed holds %d", want);
			}
			CHECK(edit_d0(col, M, d, cap) == std::min(lev(W, tq), cap), "D[0] at depth %d", d);
			for (int c0 = 0; c0 <= 1; ++c0) CHECK(edit_live(col, needs, c0, E) == (c0 + best <= E), "live at depth %d", d);
			if (d > M + E) CHECK(!edit_live(col, needs, 0, E), "a word longer than M + max_ed is live");
			++n;
		}
	}
	CHECK(small > 20000 && capped > 20000 && none > 20000, "weak cases: %ld small, %ld capped, %ld without a cell", small, capped, none);
	return n;
}

// ---- the search over tiny sets of strings ----
struct Texts {
	std::vector<std::string> s;                                // symbols as the characters 1 .. 5
	std::map<std::string, int64_t> id;
	std::vector<std::string> word;
	std::map<std::string, int64_t> memo;
	static const int64_t BIG = 1 << 20;
	int64_t N = 0, calls = 0;
	int64_t count(const std::string &w)
	{
		auto it = memo.find(w);
		if (it != memo.end()) return it->second;
		int64_t c = 0;
		for (const std::string &t : s)
			for (size_t i = 0; i + w.size() <= t.size(); ++i) c += t.compare(i, w.size(), w) == 0;
		return memo[w] = c;
	}
	void reset() { id.clear(); word.clear(); id[""] = 0; word.push_back(""); }
	void step(int64_t lo, int64_t hi, int c, int64_t &nlo, int64_t &nhi)   // the interval of a word is (id * BIG, id * BIG + occurrences), the empty word (0, N)
	{
		const std::string &w = word[(size_t)(lo / BIG)];
		CHECK(hi - lo == (w.empty() ? N : count(w)), "the bound handed back an interval it was not given");
		const std::string nw = std::string(1, (char)c) + w;
		if (!id.count(nw)) { id[nw] = (int64_t)word.size(); word.push_back(nw); }
		nlo = id[nw] * BIG; nhi = nlo + count(nw);
	}
};

struct Search {
	Texts &T;
	const uint8_t *q;
	int L, E;
	int64_t min_occ;
	const uint8_t *G;                                          // NULL: without the bound
	int pieces;
	const uint8_t *Gb;                                         // the bound that is only held against the matches below (with G == NULL)
	int pieces_b;
	std::map<std::string, int> out;
	long nodes = 0, pruned = 0, deepest = 0;

	// the node of the word W (its last symbol z, W' in front of it) at depth d with its column: the matches found at it and below it
	long node(const std::string &W, int64_t d, uint64_t col, int c0)
	{
		const int64_t M = L - 2;
		const int cap = E + 1;
		long found = 0;
		++nodes;
		deepest = std::max<long>(deepest, (long)W.size());
		CHECK((int64_t)W.size() <= L - 1 + E && (int64_t)W.size() + 1 <= edit_nodes(L, E), "a path of %zu nodes for L = %d, max_ed = %d", W.size(), L, E);
		const uint64_t win = edit_window(q, M, d + 1), needs = edit_needs(G, pieces, M, d + 1);
		for (int a = 1; a <= 4; ++a) {
			const std::string S = std::string(1, (char)a) + W;
			++T.calls;
			if (T.count(S) < min_occ) continue;
			const int e = edit_terminal(col, M, d, cap, c0, a, q[0]);
			if (e <= E) { CHECK(!out.count(S), "a word met twice"); out[S] = e; ++found; }
			const uint64_t nc = edit_step(col, win, a, cap);
			if (!edit_live(nc, needs, c0, E)) continue;
			const long below = node(S, d + 1, nc, c0);
			if (Gb && !edit_live(nc, edit_needs(Gb, pieces_b, M, d + 1), c0, E)) { ++pruned; CHECK(below == 0, "the bound prunes a node with %ld matches below it", below); }
			found += below;
		}
		return found;
	}

	void run()
	{
		const int64_t M = L - 2;
		const int cap = E + 1;
		for (int z = 1; z <= 4; ++z) {
			const std::string W(1, (char)z);
			++T.calls;
			if (T.count(W) < min_occ) continue;
			const int c0 = edit_sub(z, q[L - 1]);
			if (L == 1) { if (c0 <= E) out[W] = c0; continue; }
			const uint64_t col = edit_init(M, cap);
			if (!edit_live(col, edit_needs(G, pieces, M, 0), c0, E)) continue;
			const long below = node(W, 0, col, c0);
			if (Gb && !edit_live(col, edit_needs(Gb, pieces_b, M, 0), c0, E)) { ++pruned; CHECK(below == 0, "the bound prunes a child of the root with %ld matches below it", below); }
		}
	}
};

static long check_search(long *matches_out, long *pruned_out)
{
	long n = 0, matches = 0, pruned = 0, over = 0, saved = 0, deepest = 0, indel = 0;
	for (int set = 0; set < 1500; ++set) {
		Texts T;
		const int ns = 1 + (int)(rnd() % 5);
		for (int k = 0; k < ns; ++k) {
			std::string t;
			const int len = (int)(rnd() % 11);
			for (int i = 0; i < len; ++i) t.push_back((char)(set % 3 == 0 ? 1 + rnd() % 2 : rnd() % 10 == 0 ? 5 : 1 + rnd() % 4));
			T.s.push_back(t);
			if (rnd() % 3 == 0) T.s.push_back(t);              // duplicates: min_occ = 2 and 3 keep something
			if (rnd() % 5 == 0) T.s.push_back(t);
		}
		for (const std::string &t : T.s) T.N += (int64_t)t.size() + 1;
		// the distinct words over A C G T of the set
		std::set<std::string> words;
		for (const std::string &t : T.s)
			for (size_t i = 0; i < t.size(); ++i)
				for (size_t l = 1; i + l <= t.size() && t[i + l - 1] != (char)5; ++l) words.insert(t.substr(i, l));
		for (int t = 0; t < 3; ++t) {
			// the query: a window of a string with edits planted, or random
			const std::string &src = T.s[rnd() % T.s.size()];
			std::string qs;
			if (t < 2 && src.size() >= 2) {
				const size_t a = rnd() % (src.size() - 1);
				qs = src.substr(a, 2 + rnd() % (src.size() - a - 1));
				for (int k = (int)(rnd() % 3); k > 0 && !qs.empty(); --k) {
					const size_t at = rnd() % qs.size();
					switch (rnd() % 3) {
					case 0: qs[at] = (char)(rnd() % 6 == 0 ? 5 : 1 + rnd() % 4); break;
					case 1: qs.erase(at, 1); break;
					default: qs.insert(at, 1, (char)(1 + rnd() % 4));
					}
				}
			} else {
				const int L = 1 + (int)(rnd() % 10);
				for (int i = 0; i < L; ++i) qs.push_back((char)(rnd() % 8 == 0 ? 5 : 1 + rnd() % 4));
			}
			if (qs.empty() || qs.size() > 10) continue;
			const int L = (int)qs.size();
			uint8_t q[16], G[16];
			for (int i = 0; i < L; ++i) q[i] = (uint8_t)qs[(size_t)i];
			const int E = (int)(rnd() % (EDIT_MAX_ED + 1));
			const int64_t min_occ = 1 + (int64_t)(rnd() % 3);
			// the definition by brute force
			std::map<std::string, int> want;
			for (const std::string &S : words) {
				const int e = ed(S, qs);
				if (e <= E && T.count(S) >= min_occ) { want[S] = e; indel += (int)S.size() != L; CHECK((int)S.size() >= L - E && (int)S.size() <= L + E, "len"); }
			}
			// the bound
			int64_t steps = 0;
			T.reset();
			const int pieces = approx_bound(q, L, T.N, min_occ, E, 1000, [&](int64_t lo, int64_t hi, int c, int64_t &nlo, int64_t &nhi) { T.step(lo, hi, c, nlo, nhi); }, G, &steps);
			CHECK(pieces >= 0 && steps <= L, "the bound");
			if (pieces > E) { CHECK(want.empty(), "%d pieces at max_ed %d, and %zu matches", pieces, E, want.size()); ++over; }
			// the trie search without the bound (which holds the bound against what lies below each node) and with it
			Search plain = {T, q, L, E, min_occ, nullptr, 0, pieces <= E ? G : nullptr, pieces, {}};
			const int64_t c_before = T.calls;
			plain.run();
			const int64_t c_plain = T.calls - c_before;
			CHECK(plain.out == want, "set %d, L %d, max_ed %d, min_occ %lld: the search finds %zu matches, the definition %zu", set, L, E, (long long)min_occ, plain.out.size(), want.size());
			if (pieces <= E) {
				Search bound = {T, q, L, E, min_occ, G, pieces, nullptr, 0, {}};
				bound.run();
				CHECK(bound.out == want, "set %d, L %d, max_ed %d, min_occ %lld: with the bound %zu matches, the definition %zu", set, L, E, (long long)min_occ, bound.out.size(), want.size());
				CHECK(bound.nodes <= plain.nodes, "the bound adds nodes");
				saved += plain.nodes - bound.nodes;
			}
			CHECK(c_plain == 4 * (plain.nodes + 1), "four children a node, and the root's");
			matches += (long)want.size(); pruned += plain.pruned; deepest = std::max(deepest, plain.deepest);
			++n;
		}
	}
	CHECK(matches > 5000 && pruned > 500 && over > 100 && saved > 1000 && deepest >= 8 && indel > 1000, "weak cases: %ld matches, %ld pruned, %ld over, %ld nodes saved, deepest %ld, %ld of another length",
	      matches, pruned, over, saved, deepest, indel);
	*matches_out = matches; *pruned_out = pruned;
	return n;
}

int main()
{
	long matches = 0, pruned = 0;
	const long a = check_launches(), b = check_columns(), c = check_search(&matches, &pruned);
	printf("EDIT PLAN OK %ld launches %ld columns %ld searches %ld matches %ld pruned\n", a, b, c, matches, pruned);
	return 0;
}
