// CPU check of csrc/rb2_scratch.h (tests/test_scratch.py): CallScope on every way out of a call -- return, exception, release_open() with a longjmp
// or with the destructors behind it, a second thread, a buffer that grew -- and Carve on the four layouts of the query host layer, written here with
// the call sites' regions, against their closed sizes.  The buffers are malloc's, so that AddressSanitizer sees every byte.  A program of its own:
// prints "SCRATCH OK scopes <checks> layouts <layouts> regions <regions>" and returns 0, or says what does not hold and returns 1.
#include <atomic>
#include <csetjmp>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "rb2_scratch.h"

struct Fatal { char msg[256]; };
[[noreturn]] static void rb2_fatal(const char *fmt, ...)
{
	Fatal f;
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(f.msg, sizeof(f.msg), fmt, ap);
	va_end(ap);
	CallScope::release_open();
	throw f;
}

static std::atomic<int> g_live{0}, g_frees{0};
static std::atomic<void*> g_last_freed{nullptr};
template <class T> struct FakeBuf {
	T *p = nullptr; size_t cap = 0;
	void ensure(size_t n)                                          // exactly n items: what lies behind them is AddressSanitizer's
	{
		if (n <= cap) return;
		T *q = (T*)malloc(n * sizeof(T));
		if (p) { memcpy(q, p, cap * sizeof(T)); free(p); } else ++g_live;
		p = q; cap = n;
	}
	void release_quiet() { if (p) { free(p); g_last_freed = p; --g_live; ++g_frees; } p = nullptr; cap = 0; }
};
typedef FakeBuf<uint8_t> Bytes;

static long g_checks = 0, g_layouts = 0, g_regions = 0;
#define REQUIRE(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

/* ---- CallScope ---- */

enum Exit { RETURN, THROW, RELEASE_THROW, RELEASE_JUMP };
static jmp_buf g_env;
static void leave(Exit how)
{
	if (how == THROW) throw 1;
	if (how == RELEASE_THROW) { CallScope::release_open(); throw 1; }          // the order on a rank's thread
	if (how == RELEASE_JUMP) { CallScope::release_open(); longjmp(g_env, 1); }   // a handler that leaves by longjmp
}
static void inner(Exit how)
{
	CallScope cs;
	Bytes &a = cs.make<Bytes>(), &b = cs.make<Bytes>();
	a.ensure(100); b.ensure(1);
	cs.make<Bytes>();                                              // (never sized: nothing to free)
	REQUIRE(g_live == 4, "%d buffers live inside two scopes", (int)g_live);
	leave(how);
}
static void outer(Exit how)
{
	CallScope cs;
	Bytes &a = cs.make<Bytes>();
	FakeBuf<int64_t> &w = cs.make<FakeBuf<int64_t>>();
	a.ensure(7); w.ensure(3);
	inner(how);
	REQUIRE(g_live == 2, "%d buffers live behind the inner scope", (int)g_live);
}
static void scope_exits()
{
	const int f0 = g_frees;
	outer(RETURN);
	REQUIRE(g_live == 0 && g_frees == f0 + 4, "a normal return leaves %d buffers", (int)g_live);
	for (Exit how : {THROW, RELEASE_THROW}) {
		const int f1 = g_frees;
		bool caught = false;
		try { outer(how); } catch (int) { caught = true; }
		REQUIRE(caught && g_live == 0 && g_frees == f1 + 4, "exit %d through two scopes leaves %d buffers after %d frees", (int)how, (int)g_live, g_frees - f1);
	}
	const int f2 = g_frees;
	if (setjmp(g_env) == 0) { outer(RELEASE_JUMP); REQUIRE(false, "the longjmp came back"); }
	REQUIRE(g_live == 0 && g_frees == f2 + 4, "release_open() and a longjmp leave %d buffers", (int)g_live);
	outer(RETURN);                                                 // the chain is empty again: new scopes open and close as before
	REQUIRE(g_live == 0, "a call behind the longjmp leaves %d buffers", (int)g_live);
}
static void scope_growth()
{
	const int f0 = g_frees;
	void *last = nullptr;
	{
		CallScope cs;
		Bytes &t = cs.make<Bytes>();
		t.ensure(16);
		memset(t.p, 1, 16);
		for (size_t n = 1 << 12; n <= (1 << 22); n <<= 5) t.ensure(n);   // the caller's reference stays good while the buffer moves
		REQUIRE(t.cap == (1 << 22) && t.p[15] == 1 && g_live == 1, "a buffer that grew");
		last = t.p;
	}
	REQUIRE(g_live == 0 && g_frees == f0 + 1 && g_last_freed == last, "a buffer that grew is freed once, at its last address");
}
static void scope_threads()
{
	std::atomic<int> stage{0};
	Bytes *theirs = nullptr;
	std::thread t([&]() {
		CallScope cs;
		Bytes &b = cs.make<Bytes>();
		b.ensure(64);
		theirs = &b;
		stage = 1;
		while (stage != 2) std::this_thread::yield();
		REQUIRE(b.p && b.cap == 64, "release_open() on another thread took this thread's buffer");
		memset(b.p, 2, 64);
	});
	while (stage != 1) std::this_thread::yield();
	{
		CallScope cs;
		cs.make<Bytes>().ensure(64);
		REQUIRE(g_live == 2, "two threads hold %d buffers", (int)g_live);
		CallScope::release_open();                                 // (what make() returned is gone with it)
		REQUIRE(theirs->p && g_live == 1, "release_open() frees the calling thread's scopes and no other's");
	}
	stage = 2;
	t.join();
	REQUIRE(g_live == 0, "the second thread's scope leaves %d buffers", (int)g_live);
}

/* ---- Carve: the layouts of rb2_query_host.h ---- */

enum { UT_CTRS = 8, CL_CTRS = 4, GR_WORDS = 16, ITEMS = 4096 };
static size_t parts(size_t n) { return (n + ITEMS - 1) / ITEMS + 1; }

struct Region { uint8_t *p; size_t bytes, align; };
static std::vector<Region> g_reg;
template <class T> static T *reg(Carve &c, size_t n) { T *p = c.take<T>(n); g_reg.push_back({(uint8_t*)p, n * sizeof(T), 8}); return p; }
/* a region cut by hand into pieces of these many items */
template <class T> static void cut(std::initializer_list<size_t> ns)
{
	Region r = g_reg.back();
	g_reg.pop_back();
	size_t at = 0;
	for (size_t n : ns) { g_reg.push_back({r.p ? r.p + at : nullptr, n * sizeof(T), at ? sizeof(T) : 8}); at += n * sizeof(T); }
	REQUIRE(at == r.bytes, "the pieces of a region have %zu bytes of its %zu", at, r.bytes);
}

static void lay_chains(Carve &c, size_t n)                         // unitig_chain_layout
{
	reg<unsigned long long>(c, UT_CTRS);
	reg<uint32_t>(c, 2 * n); cut<uint32_t>({n, n});                // outdeg, indeg
	reg<int64_t>(c, 2 * n);
	reg<int64_t>(c, n);
	for (int i = 0; i < 2; ++i) reg<int64_t>(c, 4 * n);
}
static void lay_text(Carve &c, size_t n)                           // unitig_text_run
{
	reg<unsigned long long>(c, UT_CTRS);
	for (int i = 0; i < 9; ++i) reg<uint64_t>(c, n);
	reg<uint64_t>(c, parts(n));
	reg<uint64_t>(c, n);
}
static void lay_clean(Carve &c, size_t n, size_t m)                // graph_clean_run
{
	lay_chains(c, n);
	reg<unsigned long long>(c, CL_CTRS);
	reg<int64_t>(c, 4 * n);
	for (int i = 0; i < 5; ++i) reg<int64_t>(c, n);
	reg<uint64_t>(c, n + 1);
	reg<int64_t>(c, m);
	reg<uint64_t>(c, parts(m > n + 1 ? m : n + 1));
	reg<uint32_t>(c, 2 * n); cut<uint32_t>({n, n});                // cls, cur
	reg<uint8_t>(c, m + 3 * n); cut<uint8_t>({m, n, n, n});        // dead, lose, a_out, a_in
}
static void lay_graph(Carve &c, size_t most)                       // string_graph_run
{
	reg<uint64_t>(c, most + 1);
	reg<uint64_t>(c, most + 1);
	reg<uint64_t>(c, parts(most + 1));
	reg<int64_t>(c, most);
	reg<unsigned long long>(c, GR_WORDS);
}

template <class T, class F> static void check_layout(const char *name, size_t n, size_t m, size_t bytes, F lay)
{
	Carve count;
	g_reg.clear();
	lay(count);
	REQUIRE(count.size() == bytes, "%s(%zu, %zu): the counting pass says %zu bytes, the closed formula %zu", name, n, m, count.size(), bytes);
	CallScope cs;
	FakeBuf<T> &buf = cs.make<FakeBuf<T>>();
	carve_in(buf, [&](Carve &c) { g_reg.clear(); lay(c); });
	REQUIRE(buf.cap * sizeof(T) == bytes, "%s(%zu, %zu): a buffer of %zu bytes for %zu", name, n, m, buf.cap * sizeof(T), bytes);
	uint8_t *base = (uint8_t*)buf.p;
	uint8_t *at = base;
	for (size_t i = 0; i < g_reg.size(); ++i) {
		const Region &r = g_reg[i];
		REQUIRE(r.p >= at && r.p + r.bytes <= base + bytes, "%s(%zu, %zu): region %zu lies outside the buffer, or in the region before it", name, n, m, i);
		REQUIRE((size_t)(r.p - base) % r.align == 0 && (uintptr_t)r.p % r.align == 0, "%s(%zu, %zu): region %zu starts at byte %zu", name, n, m, i, (size_t)(r.p - base));
		REQUIRE((size_t)(r.p - at) < 8, "%s(%zu, %zu): %zu bytes of padding in front of region %zu", name, n, m, (size_t)(r.p - at), i);
		at = r.p + r.bytes;
		memset(r.p, (int)(i + 1), r.bytes);
	}
	for (size_t i = 0; i < g_reg.size(); ++i)
		for (size_t k = 0; k < g_reg[i].bytes; ++k)
			if (g_reg[i].p[k] != (uint8_t)(i + 1)) REQUIRE(false, "%s(%zu, %zu): byte %zu of region %zu was written by region %d", name, n, m, k, i, g_reg[i].p[k] - 1);
	++g_layouts; g_regions += (long)g_reg.size();
}

static void carve_layouts()
{
	for (size_t n : {0, 1, 2, 3, 4097}) {
		check_layout<uint8_t>("chains", n, 0, (UT_CTRS + 12 * n) * 8, [&](Carve &c) { lay_chains(c, n); });
		check_layout<uint8_t>("text", n, 0, (UT_CTRS + 10 * n + parts(n)) * 8, [&](Carve &c) { lay_text(c, n); });
		check_layout<int64_t>("graph", n, 0, (3 * n + 2 + parts(n + 1) + GR_WORDS) * 8, [&](Carve &c) { lay_graph(c, n); });
		for (size_t m : {0, 1, 5, 4096}) {
			const size_t chain_words = UT_CTRS + 12 * n, words = CL_CTRS + 11 * n + 1 + m + parts(m > n + 1 ? m : n + 1);
			check_layout<uint8_t>("clean", n, m, (chain_words + words) * 8 + (m + 3 * n), [&](Carve &c) { lay_clean(c, n, m); });
		}
	}
}
static void carve_faults()
{
	int pass = 0;
	bool said = false;
	try {
		CallScope cs;
		carve_in(cs.make<Bytes>(), [&](Carve &c) { c.take<uint64_t>(4 + (size_t)pass++); });
	} catch (const Fatal &f) { said = strstr(f.msg, "internal") != nullptr; }
	REQUIRE(said && g_live == 0, "a layout whose two passes differ is not reported");
	uint64_t word = 0;
	for (void *base : {(void*)nullptr, (void*)&word}) {
		Carve c(base);
		c.take<uint64_t>(1);
		REQUIRE(c.size() == 8, "one word");
		REQUIRE(c.take<uint64_t>(SIZE_MAX / 4) == nullptr && c.size() == Carve::SAT, "2^62 words wrap to %zu bytes", c.size());
		REQUIRE(c.take<uint8_t>(1) == nullptr && c.size() == Carve::SAT, "a saturated layout goes on counting");
		Carve d(base);
		d.take<uint8_t>(3);
		REQUIRE(d.take<uint8_t>(SIZE_MAX - 1) == nullptr && d.size() == Carve::SAT, "3 + (2^64 - 2) bytes wrap to %zu", d.size());
		Carve e(base);
		REQUIRE(e.take<uint32_t>(Carve::SAT / 4) == base && e.size() == Carve::SAT && Carve::SAT % 8 == 0, "the largest layout there is");
	}
}

int main()
{
	scope_exits();
	scope_growth();
	scope_threads();
	carve_layouts();
	carve_faults();
	printf("SCRATCH OK scopes %ld layouts %ld regions %ld\n", g_checks, g_layouts, g_regions);
	return 0;
}
