// align_stepper_host.cpp -- AlignStepper (revo_align_host.h), the Gauss-Newton loop turned inside out for revo_map_tsdf_track_many
// (DESIGN 31), held against align_loop_over itself: both are driven over the same synthetic record sequences and must give the
// same poses, bit for bit, the same iteration counts and statuses, and ask for the same evaluations at the same poses.  With it
// the rules of revo_tsdf_many_host.h that need no device: how a block finds its job, when two volumes share memory, the
// workgroups of a pose.  Stand-alone: exit code 0 and one line per sequence; test_multi_surface_cpu.py builds it with the host
// sanitizers where the toolchain has them.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../revo_amd/csrc/revo_align_host.h"
#include "../../revo_amd/csrc/revo_tsdf_many_host.h"

typedef revo_map_tsdf_track_info Rec;

static int failures = 0;
#define CHECK(cond, ...)                                                                  \
  do {                                                                                    \
    if (!(cond)) { ++failures; printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

static void fill(const Rec* r, double* H, double* g) { align_df_system_fill(reinterpret_cast<const revo_map_df_align_info*>(r), H, g); }

// A record whose system is well conditioned: H = diag(d) (S holds its upper triangle row by row), g as given.
static Rec record(const double d[6], const double g[6], uint64_t matched, int flags) {
  Rec r;
  memset(&r, 0, sizeof(r));
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) r.S[k++] = i == j ? (float)d[i] : 0.0f;
  for (int i = 0; i < 6; ++i) r.S[21 + i] = (float)g[i];
  r.matched = matched;
  r.flags = flags;
  return r;
}

struct Sequence {
  const char* name;
  std::vector<Rec> recs;  // the record of evaluation k; the last one repeats
  revo_map_align_opts o;
  int want_status, want_iterations;
};

struct Trace {
  std::vector<std::vector<float>> asked;  // the poses evaluated, in order
  float T[16];
  Rec rec;
  int it, st, rc;
};

static const Rec& nth(const Sequence& s, size_t k) { return s.recs[k < s.recs.size() ? k : s.recs.size() - 1]; }

static Trace run_loop(const Sequence& s, const float* T0, const float* centre) {
  Trace t{};
  size_t k = 0;
  t.it = -1; t.st = -1;
  t.rc = align_loop_over<Rec>(T0, centre, s.o, fill,
                              [&](const float* Tf, Rec* out) {
                                t.asked.emplace_back(Tf, Tf + 16);
                                *out = nth(s, k++);
                                memcpy(out->R, Tf, 9 * sizeof(float));  // as an evaluator does: the record names its pose
                                return 0;
                              },
                              t.T, &t.rec, &t.it, &t.st);
  return t;
}

static Trace run_stepper(const Sequence& s, const float* T0, const float* centre) {
  Trace t{};
  AlignStepper<Rec> st;
  st.begin(T0, centre, s.o);
  size_t k = 0;
  while (st.wants()) {
    const float* Tf = st.pose();
    t.asked.emplace_back(Tf, Tf + 16);
    Rec r = nth(s, k++);
    memcpy(r.R, Tf, 9 * sizeof(float));
    st.feed(r, fill);
  }
  memcpy(t.T, st.pose(), sizeof(t.T));
  t.rec = st.rec; t.it = st.it; t.st = st.st; t.rc = 0;
  CHECK((size_t)st.evals == k, "%s: evals %d, fed %zu", s.name, st.evals, k);
  return t;
}

int main() {
  const double d1[6] = {400, 500, 600, 90, 80, 70};
  const double big[6] = {8.0, -6.0, 4.0, 0.9, -0.8, 0.7}, tiny[6] = {1e-9, -1e-9, 1e-9, 1e-10, 1e-10, -1e-10}, zero[6] = {0, 0, 0, 0, 0, 0};
  const double flat[6] = {400, 500, 0, 90, 80, 70};  // a pivot that fails: rank-deficient
  const revo_map_align_opts dflt{30, 0, 1e-6, 1e-6, 12};
  std::vector<Sequence> seqs;
  seqs.push_back({"converged at the first step", {record(d1, tiny, 100, 0)}, dflt, REVO_ALIGN_CONVERGED, 1});
  seqs.push_back({"converged at a zero step", {record(d1, zero, 100, 0)}, dflt, REVO_ALIGN_CONVERGED, 1});
  seqs.push_back({"converged after three steps", {record(d1, big, 100, 0), record(d1, big, 90, 0), record(d1, tiny, 80, 0)}, dflt, REVO_ALIGN_CONVERGED, 3});
  seqs.push_back({"the iteration limit", {record(d1, big, 100, 0)}, revo_map_align_opts{4, 0, 1e-6, 1e-6, 12}, REVO_ALIGN_ITER_LIMIT, 4});
  seqs.push_back({"the iteration limit of one", {record(d1, big, 100, 0)}, revo_map_align_opts{1, 0, 1e-6, 1e-6, 12}, REVO_ALIGN_ITER_LIMIT, 1});
  seqs.push_back({"converged at the limit", {record(d1, big, 100, 0), record(d1, tiny, 100, 0)}, revo_map_align_opts{2, 0, 1e-6, 1e-6, 12}, REVO_ALIGN_CONVERGED, 2});
  seqs.push_back({"lost at the first pivot", {record(flat, big, 100, 0)}, dflt, REVO_ALIGN_LOST, 0});
  seqs.push_back({"lost for too few matches", {record(d1, big, 11, 0)}, dflt, REVO_ALIGN_LOST, 0});
  seqs.push_back({"lost after two steps", {record(d1, big, 100, 0), record(d1, big, 100, 0), record(flat, big, 100, 0)}, dflt, REVO_ALIGN_LOST, 2});
  seqs.push_back({"a record without an evaluation", {record(d1, big, 100, 1)}, dflt, REVO_ALIGN_LOST, 0});
  seqs.push_back({"a record without an evaluation after a step", {record(d1, big, 100, 0), record(d1, big, 100, 1)}, dflt, REVO_ALIGN_LOST, 1});

  const float T0[16] = {0.9998f, 0.02f, 0.0f, 0.0f, -0.02f, 0.9998f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.1f, -0.2f, 1.5f, 1.0f};
  const float centre[3] = {0.25f, -0.5f, 1.75f};
  for (const Sequence& s : seqs) {
    const Trace a = run_loop(s, T0, centre), b = run_stepper(s, T0, centre);
    CHECK(a.rc == 0 && b.rc == 0, "%s", s.name);
    CHECK(a.st == s.want_status && a.it == s.want_iterations, "%s: the loop itself gives %d after %d", s.name, a.st, a.it);
    CHECK(a.st == b.st && a.it == b.it, "%s: status %d / %d, iterations %d / %d", s.name, a.st, b.st, a.it, b.it);
    CHECK(memcmp(a.T, b.T, sizeof(a.T)) == 0, "%s: T_out differs", s.name);
    CHECK(memcmp(&a.rec, &b.rec, sizeof(Rec)) == 0, "%s: the closing record differs", s.name);
    CHECK(a.asked.size() == b.asked.size(), "%s: %zu / %zu evaluations", s.name, a.asked.size(), b.asked.size());
    for (size_t k = 0; k < a.asked.size() && k < b.asked.size(); ++k)
      CHECK(memcmp(a.asked[k].data(), b.asked[k].data(), 16 * sizeof(float)) == 0, "%s: evaluation %zu at another pose", s.name, k);
    CHECK((int)a.asked.size() == a.it + (a.st == REVO_ALIGN_LOST ? 2 : 1), "%s: %zu evaluations for %d iterations", s.name, a.asked.size(), a.it);
    CHECK(memcmp(a.T, a.asked.back().data(), sizeof(a.T)) == 0, "%s: T_out is not the last pose evaluated", s.name);
    printf("%s: status %d iterations %d evaluations %zu\n", s.name, b.st, b.it, b.asked.size());
  }

  // how a block finds its job: every block of every table, against the table walked from the front
  const std::vector<std::vector<size_t>> tables = {{8}, {1, 1, 1}, {8, 7, 105, 512, 35937}, {35937, 512, 105, 7, 8}, std::vector<size_t>(65, 3), {1u << 20, 1, 1025, 1024, 4096}};
  for (const auto& cells : tables) {
    std::vector<unsigned> first;
    unsigned total = 0;
    for (size_t c : cells) { first.push_back(total); total += tsdf_many_blocks(c); CHECK(tsdf_many_blocks(c) >= 1 && (size_t)tsdf_many_blocks(c) * 1024 >= c && ((size_t)tsdf_many_blocks(c) - 1) * 1024 < c, "blocks of %zu cells", c); }
    int want = 0;
    for (unsigned b = 0; b < total; ++b) {
      while (want + 1 < (int)first.size() && first[want + 1] <= b) ++want;
      const int got = tsdf_many_find((int)first.size(), b, [&](int j) { return first[j]; });
      CHECK(got == want, "block %u: job %d, not %d", b, got, want);
    }
  }
  // volumes that share a byte
  typedef std::vector<std::pair<uintptr_t, size_t>> Ranges;
  Ranges apart = {{4096, 64}, {1024, 3072}, {4160, 16}}, touching = {{4096, 64}, {4100, 1}}, nested = {{1024, 4096}, {8192, 8}, {2048, 8}}, same = {{64, 8}, {64, 8}};
  CHECK(!tsdf_many_overlap(apart), "apart");
  CHECK(tsdf_many_overlap(touching) && tsdf_many_overlap(nested) && tsdf_many_overlap(same), "overlaps");
  // the workgroups of a pose: revo_map_tsdf_track_eval's rule
  CHECK(tsdf_many_groups(12, 1, 0, 1024, 16384) == 12 && tsdf_many_groups(5000, 1, 0, 1024, 16384) == 1024 && tsdf_many_groups(300, 4096, 0, 1024, 16384) == 4 &&
        tsdf_many_groups(12, 65, 3, 1024, 16384) == 3 && tsdf_many_groups(1, 1, 0, 1024, 16384) == 1 && tsdf_many_groups(12, 4096, 1000, 1024, 16384) == 4, "groups");
  printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
