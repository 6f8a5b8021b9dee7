// Check of the irreducible-overlap part of csrc/rb2_query_plan.h, the arithmetic of rb2_hip_irreducible that needs no GPU: the entries a row's
// stack can hold, the bytes of a row and where its four arrays lie in them, and the rows of a launch.  Built and run by
// tests/test_irreducible_abi.py, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer; prints "IRRED PLAN OK" and
// leaves with 0 when every property holds.
#include <cstdio>
#include <cstdlib>
#include "rb2_query_plan.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// the entry cap at its edges
static long check_cap()
{
	long n = 0;
	CHECK(irred_entry_cap(100, 30, 50, 1 << 16) == 70 * 51, "reads of 100");
	CHECK(irred_entry_cap(100, 30, 50, 3569) == 3569 && irred_entry_cap(100, 30, 50, 3570) == 3570 && irred_entry_cap(100, 30, 50, 3571) == 3570, "max_steps around the product");
	CHECK(irred_entry_cap(100, 99, 1, 1000) == 2 && irred_entry_cap(100, 100, 1, 1000) == 1 && irred_entry_cap(100, 101, 8192, 1000) == 1, "no overlap length left: one entry all the same");
	CHECK(irred_entry_cap(1, 1, 1, 1) == 1 && irred_entry_cap(2, 1, 1, 1) == 1 && irred_entry_cap(2, 1, 1, 2) == 2 && irred_entry_cap(2, 1, 1, 3) == 2, "the smallest");
	CHECK(irred_entry_cap(IRRED_MAX_LEN, 1, IRRED_MAX_LEN, INT64_MAX) == (IRRED_MAX_LEN - 1) * (IRRED_MAX_LEN + 1), "the largest");
	CHECK(irred_entry_cap(IRRED_MAX_LEN, INT64_MAX, IRRED_MAX_LEN, INT64_MAX) == 1 && irred_entry_cap(IRRED_MAX_LEN, 1, IRRED_MAX_LEN, 1 << 16) == 1 << 16, "min_ovlp and max_steps at their ends");
	const int64_t lens[] = {1, 2, 3, 20, 101, 4096, 8191, 8192}, ovs[] = {1, 2, 19, 20, 21, 100, 101, 8191, 8192, 8193, (int64_t)1 << 40},
	              exts[] = {1, 2, 7, 100, 8191, 8192}, stepss[] = {1, 2, 7, 40, 1000, 1 << 16, (int64_t)1 << 30, INT64_MAX};
	for (int64_t L : lens) for (int64_t mo : ovs) for (int64_t me : exts) for (int64_t ms : stepss) {
		const int64_t cap = irred_entry_cap(L, mo, me, ms), per = L > mo ? L - mo : 0, nf = irred_frames(cap, me), rb = irred_row_bytes(cap, me);
		CHECK(cap >= 1 && cap <= (ms > 1 ? ms : 1) && (per == 0 ? cap == 1 : cap <= per * (me + 1)), "cap %lld", (long long)cap);
		CHECK(cap == ms || cap == per * (me + 1) || (cap == 1 && per == 0), "L %lld min_ovlp %lld max_ext %lld max_steps %lld: cap %lld is neither bound", (long long)L, (long long)mo, (long long)me, (long long)ms, (long long)cap);
		// a path of frames 0 .. max_ext with per entries each fits unless max_steps ends the query first
		CHECK(cap >= (per * (me + 1) < ms ? per * (me + 1) : ms) || per == 0, "cap too small");
		CHECK(nf >= 1 && nf <= cap && nf <= me, "frames %lld", (long long)nf);
		// the arrays of a row as k_irreducible lays them out: kid, fs, el, fa, each on an 8-byte boundary, the last one ending inside the row
		const int64_t o_fs = 64 * cap, o_el = o_fs + irred_pad(4 * nf), o_fa = o_el + irred_pad(2 * cap), end = o_fa + nf;
		CHECK(o_fs % 8 == 0 && o_el % 8 == 0 && o_fa % 8 == 0 && o_el >= o_fs + 4 * nf && o_fa >= o_el + 2 * cap, "the arrays overlap");
		CHECK(end <= rb && rb < end + 8 && rb % 8 == 0 && rb >= 66 * cap + 5 * nf && rb <= 66 * cap + 5 * nf + 21, "row bytes %lld", (long long)rb);
		++n;
	}
	CHECK(irred_row_bytes(1, 1) == 64 + 8 + 8 + 8 && irred_row_bytes(4, 4) == 256 + 16 + 8 + 8 && irred_row_bytes(70 * 51, 50) == 64 * 3570 + 200 + 7144 + 56, "row bytes");
	CHECK(irred_pad(0) == 0 && irred_pad(1) == 8 && irred_pad(8) == 8 && irred_pad(9) == 16, "pad");
	return n;
}

// the rows of a launch
static long check_rows()
{
	long n = 0;
	const int64_t sizes[] = {1, 87, 88, 89, 175, 176, 177, 4096, 1 << 20, IRRED_SCRATCH_BYTES}, ns[] = {1, 2, 15, 16, 17, 300, 32767, 32768, 32769, 1 << 20};
	const int64_t rbs[] = {88, 96, 1000, 235800, (int64_t)1 << 28, ((int64_t)1 << 28) + 8, (int64_t)1 << 32};
	for (int64_t bytes : sizes) for (int64_t nq : ns) for (int64_t rb : rbs) {
		const int64_t r = stack_rows(nq, rb, bytes, IRRED_ROWS);
		CHECK(r >= 1 && r <= nq && r <= IRRED_ROWS, "rows");
		CHECK(r == 1 || r * rb <= bytes, "n %lld row %lld bytes %lld: %lld rows do not fit", (long long)nq, (long long)rb, (long long)bytes, (long long)r);
		CHECK(r == nq || r == IRRED_ROWS || (r + 1) * rb > bytes, "n %lld row %lld bytes %lld: %lld rows could be more", (long long)nq, (long long)rb, (long long)bytes, (long long)r);
		++n;
	}
	CHECK(stack_rows(100, 88, 176, IRRED_ROWS) == 2 && stack_rows(100, 88, 175, IRRED_ROWS) == 1 && stack_rows(100, 88, 1, IRRED_ROWS) == 1 && stack_rows(1 << 20, 88, IRRED_SCRATCH_BYTES, IRRED_ROWS) == IRRED_ROWS, "rows at the edges");
	CHECK(stack_rows(1000000, irred_row_bytes(irred_entry_cap(100, 50, 50, 1 << 16), 50), IRRED_SCRATCH_BYTES, IRRED_ROWS) == 1592, "reads of 100 at min_ovlp 50");
	return n;
}

int main()
{
	const long a = check_cap(), b = check_rows();
	printf("IRRED PLAN OK %ld caps %ld rows\n", a, b);
	return 0;
}
