// The bit arithmetic of string deletion (rb2_hip_delete_strings: kernels in rb2_delete.h) that needs no GPU: the
// compress of a group's bit planes by its kept mask, and where the kept bits of a group go in the destination piece.  Plain C++, marked
// for both sides when a HIP compiler reads it, so that a CPU program can include it (tests/test_delete_plan.py).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define RB2_DEL_HD __host__ __device__ __forceinline__
#else
#define RB2_DEL_HD inline
#endif

/* the layout of a leaf as rb2_device.h has it: 16 groups of 64 symbols, three bit planes, plane-major */
static const uint32_t DEL_GSYM = 64, DEL_LEAFG = 16, DEL_LEAFW = 48, DEL_LEAF_SH = 10;

/* Software bit compress (the "compress" of Hacker's Delight 7-4, 64 bits wide): the bits of x where m is set, packed to the low end in
 * their order.  What depends on the mask alone -- the six move masks -- is computed once (del_compress_plan) and applied to the three
 * planes of a group (del_compress). */
struct DelCompress { uint64_t m, mv[6]; };

RB2_DEL_HD DelCompress del_compress_plan(uint64_t m)
{
	DelCompress P;
	P.m = m;
	uint64_t mk = ~m << 1;                                     /* the zeros to the right of every bit are counted */
	for (int i = 0; i < 6; ++i) {
		uint64_t mp = mk ^ (mk << 1);                          /* parallel prefix: bit k = parity of the zeros below k */
		mp ^= mp << 2; mp ^= mp << 4; mp ^= mp << 8; mp ^= mp << 16; mp ^= mp << 32;
		const uint64_t mv = mp & m;                            /* the bits that move by 2^i in this stage */
		P.mv[i] = mv;
		m = (m ^ mv) | (mv >> (1u << i));                      /* the mask is compressed along with the data */
		mk &= ~mp;
	}
	return P;
}

RB2_DEL_HD uint64_t del_compress(const DelCompress &P, uint64_t x)
{
	x &= P.m;
	for (int i = 0; i < 6; ++i) {
		const uint64_t t = x & P.mv[i];
		x = (x ^ t) | (t >> (1u << i));
	}
	return x;
}

/* a kept mask whose set bits are the low ones needs no compress: the kept bits of a plane are plane & m, already in place (the group
 * lost no row, or only rows behind its last kept one) */
RB2_DEL_HD bool del_mask_is_prefix(uint64_t m) { return (m & (m + 1)) == 0; }

/* Where c kept bits (0 <= c <= 64), packed to the low end of a word, go when the first of them is row d of a destination piece whose
 * first leaf is leaf0: OR (bits << shift) into 64-bit word `word` of the pool (plane pl of the group that holds row d) and, when
 * spill is set, (bits >> (64 - shift)) into word `word2` -- the same plane of the next group, which is in the next leaf when the
 * group of d is its leaf's last. */
struct DelDst { uint64_t word, word2; uint32_t shift; bool spill; };

RB2_DEL_HD uint64_t del_plane_word(uint64_t leaf0, uint64_t d, uint32_t pl)
{
	return (leaf0 + (d >> DEL_LEAF_SH)) * DEL_LEAFW + (uint64_t)pl * DEL_LEAFG + ((d >> 6) & (DEL_LEAFG - 1));
}

RB2_DEL_HD DelDst del_dst(uint64_t leaf0, uint64_t d, uint32_t c, uint32_t pl)
{
	DelDst D;
	D.shift = (uint32_t)(d & (DEL_GSYM - 1));
	D.word = del_plane_word(leaf0, d, pl);
	D.spill = D.shift + c > DEL_GSYM;
	D.word2 = del_plane_word(leaf0, (d | (DEL_GSYM - 1)) + 1, pl);
	return D;
}
