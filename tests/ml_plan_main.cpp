// Stand-alone driver of the host planner (csrc/ml_plan.cpp) for tests/test_ml_plan.py, which builds it together with
// tuning.cpp and dist_plan.cpp under the address and undefined-behaviour sanitizers: no HIP runtime, no Python.
//
//    ml_plan_main matrix.bin coarsest_rows
//
// matrix.bin: int64 n, nnz, nblk, geo; int32 rowptr[n + 1], colind[nnz]; double val[nnz]; int32 blk_start[nblk + 1],
// col_i[nblk], col_j[nblk] (passed on only if geo).  Prints "levels <rows of every level>", then the sha256 of rows (int64)
// and of every level's cmap and col_of (int32).
#include "../include/nkp.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

// SHA-256 (FIPS 180-4) of a byte range, as lower-case hex
static std::string sha256 (const void *data, size_t len)
{
   static const uint32_t k[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
      0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
      0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
      0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
      0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2 };
   uint32_t h[8] = { 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19 };
   std::vector<unsigned char> m ((const unsigned char *) data, (const unsigned char *) data + len);
   m.push_back (0x80);
   while (m.size () % 64 != 56) m.push_back (0);
   for (int s = 56; s >= 0; s -= 8) m.push_back ((unsigned char) (((uint64_t) len * 8) >> s));
   auto rotr = [] (uint32_t x, int s) { return (x >> s) | (x << (32 - s)); };
   for (size_t off = 0; off < m.size (); off += 64) {
      uint32_t w[64];
      for (int i = 0; i < 16; i++)
         w[i] = (uint32_t) m[off + 4 * i] << 24 | (uint32_t) m[off + 4 * i + 1] << 16 | (uint32_t) m[off + 4 * i + 2] << 8 | (uint32_t) m[off + 4 * i + 3];
      for (int i = 16; i < 64; i++) {
         const uint32_t s0 = rotr (w[i - 15], 7) ^ rotr (w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr (w[i - 2], 17) ^ rotr (w[i - 2], 19) ^ (w[i - 2] >> 10);
         w[i] = w[i - 16] + s0 + w[i - 7] + s1;
      }
      uint32_t v[8];
      memcpy (v, h, sizeof v);
      for (int i = 0; i < 64; i++) {
         const uint32_t t1 = v[7] + (rotr (v[4], 6) ^ rotr (v[4], 11) ^ rotr (v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) + k[i] + w[i];
         const uint32_t t2 = (rotr (v[0], 2) ^ rotr (v[0], 13) ^ rotr (v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
         for (int q = 7; q > 0; q--) v[q] = v[q - 1];
         v[4] += t1;
         v[0] = t1 + t2;
      }
      for (int q = 0; q < 8; q++) h[q] += v[q];
   }
   char hex[65];
   for (int q = 0; q < 8; q++) snprintf (hex + 8 * q, 9, "%08x", h[q]);
   return hex;
}

template <class T>
static std::vector<T> read_array (FILE *f, size_t count)
{
   std::vector<T> v (count);
   if (fread (v.data (), sizeof (T), count, f) != count) { fprintf (stderr, "ml_plan_main: short read\n"); exit (2); }
   return v;
}

int main (int argc, char **argv)
{
   if (argc != 3) { fprintf (stderr, "usage: ml_plan_main matrix.bin coarsest_rows\n"); return 2; }
   FILE *f = fopen (argv[1], "rb");
   if (!f) { fprintf (stderr, "ml_plan_main: cannot open %s\n", argv[1]); return 2; }
   const std::vector<int64_t> head = read_array<int64_t> (f, 4);
   const int64_t n = head[0], nnz = head[1], nblk = head[2];
   const bool geo = head[3] != 0;
   const std::vector<int32_t> rowptr = read_array<int32_t> (f, (size_t) n + 1), colind = read_array<int32_t> (f, (size_t) nnz);
   const std::vector<double> val = read_array<double> (f, (size_t) nnz);
   const std::vector<int32_t> blk = read_array<int32_t> (f, (size_t) nblk + 1), ci = read_array<int32_t> (f, (size_t) nblk), cj = read_array<int32_t> (f, (size_t) nblk);
   fclose (f);
   const int64_t cap = 2 * n + 64;
   std::vector<int32_t> cmap ((size_t) cap), col_of ((size_t) cap);
   std::vector<int64_t> rows (64);
   int nlev = 0;
   const int rc = nkp_ml_plan_host (n, rowptr.data (), colind.data (), val.data (), blk.data (), nblk, geo ? ci.data () : nullptr, geo ? cj.data () : nullptr, 1, 0,
                                    atoi (argv[2]), cap, &nlev, rows.data (), cmap.data (), col_of.data ());
   if (rc) { fprintf (stderr, "ml_plan_main: nkp_ml_plan_host returned %d (%s)\n", rc, nkp_last_error ()); return 1; }
   printf ("levels");
   for (int l = 0; l < nlev; l++) printf (" %lld", (long long) rows[(size_t) l]);
   printf ("\nrows %s\n", sha256 (rows.data (), (size_t) nlev * sizeof (int64_t)).c_str ());
   int64_t qc = 0, qo = 0;
   for (int l = 0; l + 1 < nlev; l++) {
      printf ("cmap %s\n", sha256 (cmap.data () + qc, (size_t) rows[(size_t) l] * sizeof (int32_t)).c_str ());
      printf ("col_of %s\n", sha256 (col_of.data () + qo, (size_t) rows[(size_t) l + 1] * sizeof (int32_t)).c_str ());
      qc += rows[(size_t) l];
      qo += rows[(size_t) l + 1];
   }
   return 0;
}
