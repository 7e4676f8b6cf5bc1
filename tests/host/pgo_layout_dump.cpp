// pgo_layout_dump — runs build_pgo_layout (csrc/pgo_layout.hpp) on a graph read from a file and writes every field of the
// layout to another: the host-only half of nos_pgo_create without a GPU (tests/test_pgo_layout_host.py; also the program
// to build with a sanitizer).  All words little-endian.
//   in : u64 n_poses, n_edges, has_switch_init, has_switch_free, has_fixed, want_blocks, max_threads;
//        f64 poses[n_poses][7]; i32 ref[n_edges], qry[n_edges]; f64 meas[n_edges][7];
//        then, each only if its flag is set: f64 switch_init[n_edges]; u8 switch_free[n_edges]; u8 fixed[n_poses]
//   out: u64 ok, bad_constraint, n_poses, n_edges, n_free_switches, n_blocks, largest_slots, largest_halo, blocks_fit;
//        then (ok only) twelve arrays, each as u64 bytes + data: pose_rec, edge_rec, sw_free, fixed, adj_off, adj, adj_nbr,
//        entry_off, halo_off, and the pieces laid end to end: entries, entry constraints, halo
// Exit status 2 when a piece does not start where entry_off / halo_off of its first block say (the upload relies on it).
#include <cstdio>
#include <cstdlib>

#include "pgo_layout.hpp"

namespace {

template <class T>
std::vector<T> read_array(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count != 0 && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "pgo_layout_dump: input too short\n");
    exit(1);
  }
  return v;
}

template <class T>
void write_array(FILE* f, const std::vector<T>& v) {
  const uint64_t bytes = v.size() * sizeof(T);
  fwrite(&bytes, sizeof bytes, 1, f);
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

// One list of the pieces end to end: the total size first, as for an array.
template <class T>
void write_pieces(FILE* f, const nos::PgoLayout& L, std::vector<T> nos::PgoLayoutPiece::*list) {
  uint64_t bytes = 0;
  for (const nos::PgoLayoutPiece& pc : L.pieces) bytes += (pc.*list).size() * sizeof(T);
  fwrite(&bytes, sizeof bytes, 1, f);
  for (const nos::PgoLayoutPiece& pc : L.pieces)
    if (!(pc.*list).empty()) fwrite((pc.*list).data(), sizeof(T), (pc.*list).size(), f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: pgo_layout_dump <graph file> <layout file>\n");
    return 1;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return perror(argv[1]), 1;
  const std::vector<uint64_t> head = read_array<uint64_t>(in, 7);
  const size_t N = head[0], M = head[1];
  const std::vector<double> poses = read_array<double>(in, 7 * N);
  const std::vector<int32_t> ref = read_array<int32_t>(in, M), qry = read_array<int32_t>(in, M);
  const std::vector<double> meas = read_array<double>(in, 7 * M);
  const std::vector<double> sw_init = read_array<double>(in, head[2] ? M : 0);
  const std::vector<unsigned char> sw_free = read_array<unsigned char>(in, head[3] ? M : 0);
  const std::vector<unsigned char> fixed = read_array<unsigned char>(in, head[4] ? N : 0);
  fclose(in);

  nos::PgoLayout L;
  const bool ok = nos::build_pgo_layout(N, poses.data(), M, ref.data(), qry.data(), meas.data(), head[2] ? sw_init.data() : nullptr,
                                        head[3] ? sw_free.data() : nullptr, head[4] ? fixed.data() : nullptr, head[5] != 0, &L,
                                        unsigned(head[6]));
  size_t n_ent = 0, n_halo = 0;
  for (const nos::PgoLayoutPiece& pc : L.pieces) {
    if (L.entry_off[pc.first_block] != n_ent || L.halo_off[pc.first_block] != n_halo || pc.ent.size() != 10 * pc.edge.size()) {
      fprintf(stderr, "pgo_layout_dump: the piece from block %u on is not where the offsets say\n", pc.first_block);
      return 2;
    }
    n_ent += pc.edge.size();
    n_halo += pc.halo.size();
  }

  FILE* out = fopen(argv[2], "wb");
  if (!out) return perror(argv[2]), 1;
  const uint64_t scalars[9] = {ok, L.bad_constraint, L.n_poses, L.n_edges, L.n_free_switches, L.n_blocks, L.largest_slots,
                               L.largest_halo, L.blocks_fit};
  fwrite(scalars, sizeof scalars, 1, out);
  if (ok) {
    write_array(out, L.pose_rec);
    write_array(out, L.edge_rec);
    write_array(out, L.sw_free);
    write_array(out, L.fixed);
    write_array(out, L.adj_off);
    write_array(out, L.adj);
    write_array(out, L.adj_nbr);
    write_array(out, L.entry_off);
    write_array(out, L.halo_off);
    write_pieces(out, L, &nos::PgoLayoutPiece::ent);
    write_pieces(out, L, &nos::PgoLayoutPiece::edge);
    write_pieces(out, L, &nos::PgoLayoutPiece::halo);
  }
  return fclose(out) == 0 ? 0 : 1;
}
