// Stand-alone host program of tests/test_dist_smooth_plan.py: the planner of the row-distributed flavour (csrc/dist_plan.cpp with
// csrc/tuning.cpp, nothing else) run on all ranks of one case at once, one thread per rank, over a communicator made of a mutex,
// a condition variable and the peers' own buffers.  Built with the address and undefined-behaviour sanitizers; prints the lists
// of the fine-level exchange (tuning dist_smooth_exchange) of every rank, one line per rank and list.
//
//    dist_smooth_plan_main CASE      CASE as tests/dist_smooth_worker.py --dump writes it: "P n nblk rings", then one line each of
//                                    starts, rowptr, colind, blk_start, col_i, col_j (integers) and the values (hex floats)
#include "../include/nkp.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <fstream>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

namespace {

struct World {
   int P = 0;
   std::mutex mu;
   std::condition_variable cv;
   int waiting = 0;
   long generation = 0;
   std::vector<const int32_t *> send;
   std::vector<const int *> scnt;
   std::vector<int64_t> value;
   void barrier ()
   {
      std::unique_lock<std::mutex> lk (mu);
      const long g = generation;
      if (++waiting == P) { waiting = 0; generation++; cv.notify_all (); }
      else cv.wait (lk, [&] { return generation != g; });
   }
};

struct Rank { World *w; int rank; };

int alltoallv_i32 (void *ctx, const int32_t *send, const int *scnt, int32_t *recv, const int *rcnt)
{
   Rank *r = (Rank *) ctx;
   World &w = *r->w;
   w.send[(size_t) r->rank] = send;
   w.scnt[(size_t) r->rank] = scnt;
   w.barrier ();
   int bad = 0;
   size_t at = 0;
   for (int p = 0; p < w.P; p++) {
      size_t off = 0;
      for (int q = 0; q < r->rank; q++) off += (size_t) w.scnt[(size_t) p][q];
      if (w.scnt[(size_t) p][r->rank] != rcnt[p]) bad = 1;      // the planner's counts must agree both ways
      else if (rcnt[p] > 0) memcpy (recv + at, w.send[(size_t) p] + off, (size_t) rcnt[p] * sizeof (int32_t));
      at += (size_t) rcnt[p];
   }
   w.barrier ();
   return bad;
}

int allgather_i64 (void *ctx, int64_t mine, int64_t *out)
{
   Rank *r = (Rank *) ctx;
   World &w = *r->w;
   w.value[(size_t) r->rank] = mine;
   w.barrier ();
   for (int p = 0; p < w.P; p++) out[p] = w.value[(size_t) p];
   w.barrier ();
   return 0;
}

template <class T>
bool read_line (std::ifstream &in, std::vector<T> &v, bool hex_float = false)
{
   std::string line;
   if (!std::getline (in, line)) return false;
   std::istringstream ss (line);
   std::string tok;
   while (ss >> tok) v.push_back (hex_float ? (T) strtod (tok.c_str (), nullptr) : (T) strtoll (tok.c_str (), nullptr, 10));
   return true;
}

}   // namespace

int main (int argc, char **argv)
{
   if (argc != 2) { fprintf (stderr, "usage: %s CASE\n", argv[0]); return 2; }
   std::ifstream in (argv[1]);
   std::vector<int64_t> head, starts;
   std::vector<int32_t> rowptr, colind, blk, ci, cj;
   std::vector<double> val;
   if (!in || !read_line (in, head) || head.size () != 4 || !read_line (in, starts) || !read_line (in, rowptr) || !read_line (in, colind) || !read_line (in, blk) ||
       !read_line (in, ci) || !read_line (in, cj) || !read_line (in, val, true)) { fprintf (stderr, "cannot read %s\n", argv[1]); return 2; }
   const int P = (int) head[0], rings = (int) head[3];
   const int64_t n = head[1], nblk = head[2];
   if ((int64_t) starts.size () != P + 1 || (int64_t) rowptr.size () != n + 1 || (int64_t) blk.size () != nblk + 1 || (int64_t) ci.size () != nblk ||
       (int64_t) cj.size () != nblk || colind.size () != val.size () || (int64_t) colind.size () != rowptr[(size_t) n]) { fprintf (stderr, "inconsistent case\n"); return 2; }
   World w;
   w.P = P;
   w.send.assign ((size_t) P, nullptr);
   w.scnt.assign ((size_t) P, nullptr);
   w.value.assign ((size_t) P, 0);
   std::vector<std::string> text ((size_t) P);
   std::vector<int> code ((size_t) P, 0);
   auto work = [&] (int rank) {
      Rank me = { &w, rank };
      const int64_t f = starts[(size_t) rank], m = starts[(size_t) rank + 1] - f;
      std::vector<int32_t> rp ((size_t) m + 1);
      for (int64_t r = 0; r <= m; r++) rp[(size_t) r] = rowptr[(size_t) (f + r)] - rowptr[(size_t) f];
      int64_t b0 = 0, b1 = 0;
      while (blk[(size_t) b0] < f) b0++;
      while (blk[(size_t) b1] < f + m) b1++;
      std::vector<int32_t> bl ((size_t) (b1 - b0) + 1);
      for (int64_t b = b0; b <= b1; b++) bl[(size_t) (b - b0)] = blk[(size_t) b] - (int32_t) f;
      nkp_tuning tune;
      nkp_default_tuning (&tune);
      tune.dist_smooth_exchange = 1;
      tune.dist_ras_rings = rings;
      nkp_options opt;
      nkp_default_options (&opt);
      opt.tuning = &tune;
      opt.col_i = ci.data () + b0;
      opt.col_j = cj.data () + b0;
      nkp_comm_ops ops;
      memset (&ops, 0, sizeof ops);
      ops.ctx = &me;
      ops.rank = rank;
      ops.nranks = P;
      ops.alltoallv_i32_host = alltoallv_i32;
      ops.allgather_i64_host = allgather_i64;
      nkp_dist_plan *pl = nullptr;
      const int64_t e0 = rowptr[(size_t) f];
      code[(size_t) rank] = nkp_dist_overlap_plan_host (&pl, &opt, n, f, m, rp[(size_t) m], rp.data (), colind.data () + e0, val.data () + e0, bl.data (), b1 - b0, 1, &ops);
      if (code[(size_t) rank]) { text[(size_t) rank] = std::string ("error ") + nkp_last_error () + "\n"; return; }
      std::ostringstream out;
      out << rank << " smooth_exchange " << nkp_dist_plan_size (pl, "smooth_exchange") << "\n";
      for (const char *name : { "smooth_send_rows0", "smooth_send_rows1", "smooth_recv_rows0", "smooth_recv_rows1", "smooth_give0", "smooth_give1", "smooth_need0", "smooth_need1" }) {
         const int64_t cnt = nkp_dist_plan_size (pl, name);
         std::vector<int32_t> v ((size_t) (cnt > 0 ? cnt : 0) + 1);
         if (cnt > 0) nkp_dist_plan_copy (pl, name, v.data ());
         out << rank << " " << name;
         for (int64_t k = 0; k < cnt; k++) out << " " << v[(size_t) k];
         out << "\n";
      }
      nkp_dist_plan_free (pl);
      text[(size_t) rank] = out.str ();
   };
   std::vector<std::thread> pool;
   for (int r = 0; r < P; r++) pool.emplace_back (work, r);
   for (std::thread &t : pool) t.join ();
   int rc = 0;
   for (int r = 0; r < P; r++) {
      fputs (text[(size_t) r].c_str (), stdout);
      if (code[(size_t) r]) rc = 1;
   }
   return rc;
}
