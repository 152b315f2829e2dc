// `verify` -- checks input.json files as the circuit does before any witness is generated (include/codex_p2.h,
// cp2_proof_inputs_verify: what SampleAndProve of circuit/codex/sample_cells.circom:58-148 accepts).
//
//   verify [--maxdepth=32] [--maxslots=256] [--cellsize=2048] [--blocksize=65536] [--nsamples=N] FILE...
//
// The circuit parameters mean what they mean for the `cli` twin (maxslots is a slot count: maxLog2NSlots = its ceiling log2);
// without --nsamples every file is read with as many samples as it has rows (files of one batch must agree).  Files are parsed on
// at most 16 host threads and verified in batches on GPU 0.  One line per file:
//   FILE: accepted  |  FILE: rejected: dataset root  |  FILE: rejected: samples 3,17  |  FILE: shape: nCellsPerSlot=3
// (samples are numbered as the rows of cellData / merklePaths, from 0: sample k is the one with counter k + 1).
// Exit status: 0 all accepted, 1 some rejected, 2 a usage, parse, I/O or device error (with the message).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/codex_p2.h"

namespace {

[[noreturn]] void usage(const std::string& why) {
  std::cerr << "verify: " << why << "\n"
            << "usage: verify [--maxdepth=32] [--maxslots=256] [--cellsize=2048] [--blocksize=65536] [--nsamples=N] FILE...\n";
  std::exit(2);
}

uint64_t parse_u64(const std::string& key, const std::string& v) {
  if (v.empty() || v.size() > 18 || v.find_first_not_of("0123456789") != std::string::npos) usage("--" + key + " takes a decimal number");
  return std::stoull(v);
}

int ceiling_log2(uint64_t x) {   // misc.nim:10-23
  int k = 0;
  while (k < 63 && (1ULL << k) < x) ++k;
  return k;
}

bool read_file(const std::string& path, std::string* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::ostringstream ss;
  ss << f.rdbuf();
  if (f.bad()) return false;
  *out = ss.str();
  return true;
}

struct Item {
  std::string path, error;   // error: parse or I/O failure (exit status 2)
  cp2_proof_input* p = nullptr;
};

}  // namespace

int main(int argc, char** argv) {
  const int v = cp2_abi_version();
  if ((v >> 16) != CP2_ABI_VERSION_MAJOR || (v & 0xffff) < CP2_ABI_VERSION_MINOR) {
    std::cerr << "verify: libcodex_p2.so has ABI version " << (v >> 16) << "." << (v & 0xffff) << ", this program was built against "
              << CP2_ABI_VERSION_MAJOR << "." << CP2_ABI_VERSION_MINOR << "\n";
    return 2;
  }
  cp2_config cfg{};
  cfg.max_depth = 32;
  cfg.max_log2_nslots = 8;
  cfg.cell_size = 2048;
  cfg.block_size = 65536;
  cfg.n_samples = 0;   // as many rows as each file has
  std::vector<std::string> files;
  for (int a = 1; a < argc; ++a) {
    const std::string arg = argv[a];
    if (arg.rfind("--", 0) != 0) {
      if (!arg.empty() && arg[0] == '-') usage("unknown option " + arg + " (long options only)");
      files.push_back(arg);
      continue;
    }
    const size_t eq = arg.find('=');
    if (eq == std::string::npos) usage("option " + arg + " needs =value");
    const std::string key = arg.substr(2, eq - 2), val = arg.substr(eq + 1);
    const uint64_t x = parse_u64(key, val);
    if (key == "maxdepth") {
      if (x > 64) usage("--maxdepth is at most 64");
      cfg.max_depth = (int32_t)x;
    } else if (key == "maxslots") {
      cfg.max_log2_nslots = ceiling_log2(x);
    } else if (key == "cellsize") {
      cfg.cell_size = x;
    } else if (key == "blocksize") {
      cfg.block_size = x;
    } else if (key == "nsamples") {
      if (x == 0) usage("--nsamples must be positive");
      cfg.n_samples = x;
    } else {
      usage("unknown option --" + key);
    }
  }
  if (files.empty()) usage("no input files");
  if (cfg.cell_size == 0 || cfg.block_size % cfg.cell_size || ((cfg.block_size / cfg.cell_size) & (cfg.block_size / cfg.cell_size - 1)) ||
      cfg.block_size / cfg.cell_size < 2)
    usage("--blocksize / --cellsize must be a power of two >= 2");

  cp2_ctx* ctx = nullptr;
  int st = cp2_init(0, &ctx);
  if (st != CP2_OK) {
    std::cerr << "verify: cp2_init: " << cp2_strerror(st) << "\n";
    return 2;
  }
  const size_t threads = std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
  constexpr size_t BATCH = 1024;
  bool rejected = false, failed = false;
  bool device_failed = false;
  for (size_t b0 = 0; b0 < files.size() && !device_failed; b0 += BATCH) {
    const size_t nb = std::min(BATCH, files.size() - b0);
    std::vector<Item> items(nb);
    std::vector<std::thread> th;
    for (size_t w = 0; w < std::min(threads, nb); ++w)
      th.emplace_back([&, w] {
        for (size_t i = w; i < nb; i += std::min(threads, nb)) {
          Item& it = items[i];
          it.path = files[b0 + i];
          std::string text;
          if (!read_file(it.path, &text)) {
            it.error = "cannot read the file";
            continue;
          }
          char msg[512] = "";
          const int s = cp2_proof_input_parse_json(&cfg, text.data(), text.size(), &it.p, msg, sizeof msg);
          if (s != CP2_OK) it.error = std::string(cp2_strerror(s)) + (msg[0] ? std::string(": ") + msg : std::string());
        }
      });
    for (auto& t : th) t.join();
    // verify the parsed files of this batch that share the first one's sample count (with --nsamples all of them do)
    std::vector<const cp2_proof_input*> ps;
    std::vector<size_t> at;
    for (size_t i = 0; i < nb; ++i)
      if (items[i].p && (ps.empty() || cp2_proof_input_nsamples(items[i].p) == cp2_proof_input_nsamples(ps[0]))) {
        ps.push_back(items[i].p);
        at.push_back(i);
      } else if (items[i].p) {
        items[i].error = "has " + std::to_string(cp2_proof_input_nsamples(items[i].p)) + " samples, the batch " +
                         std::to_string(cp2_proof_input_nsamples(ps[0])) + " (give --nsamples)";
      }
    const size_t ns = ps.empty() ? 0 : cp2_proof_input_nsamples(ps[0]);
    std::vector<uint32_t> status(ps.size());
    std::vector<uint8_t> ok(ps.size() * ns);
    if (!ps.empty()) {
      st = cp2_proof_inputs_verify(ctx, ps.data(), ps.size(), status.data(), ok.data());
      if (st != CP2_OK) {
        std::cerr << "verify: cp2_proof_inputs_verify: " << cp2_strerror(st) << " (" << cp2_last_error(ctx) << ")\n";
        device_failed = true;
      }
    }
    std::vector<int> row(nb, -1);
    for (size_t j = 0; j < at.size(); ++j) row[at[j]] = (int)j;
    for (size_t i = 0; i < nb && !device_failed; ++i) {
      const Item& it = items[i];
      if (!it.error.empty()) {
        std::cout << it.path << ": error: " << it.error << "\n";
        failed = true;
        continue;
      }
      const size_t j = (size_t)row[i];
      const uint32_t s = status[j];
      if (s == 0) {
        std::cout << it.path << ": accepted\n";
        continue;
      }
      rejected = true;
      if (s & CP2_VERIFY_SHAPE) {   // what witness generation refuses (lib/log2.circom, misc.circom ToBits), by the values the file states
        uint64_t nc = 0, nsl = 0, si = 0;
        (void)cp2_proof_input_shape(it.p, &nc, &nsl, &si);
        const int lg = (nc && !(nc & (nc - 1))) ? __builtin_ctzll(nc) : -1;
        const uint64_t lim = 1ULL << cfg.max_log2_nslots;
        std::cout << it.path << ": shape:";
        if (lg < 1 || lg > cfg.max_depth) std::cout << " nCellsPerSlot=" << nc;
        if (nsl == 0 || nsl - 1 >= lim) std::cout << " nSlotsPerDataSet=" << nsl;
        if (si >= lim) std::cout << " slotIndex=" << si;
        std::cout << "\n";
        continue;
      }
      std::cout << it.path << ": rejected:";
      if (s & CP2_VERIFY_DATASET_ROOT) std::cout << " dataset root" << ((s & CP2_VERIFY_SAMPLE) ? ";" : "");
      if (s & CP2_VERIFY_SAMPLE) {
        std::cout << " samples ";
        bool first = true;
        for (size_t k = 0; k < ns; ++k)
          if (!ok[j * ns + k]) {
            std::cout << (first ? "" : ",") << k;
            first = false;
          }
      }
      std::cout << "\n";
    }
    for (auto& it : items) cp2_proof_input_free(it.p);
  }
  std::cout.flush();
  cp2_free(ctx);
  return (failed || device_failed) ? 2 : rejected ? 1 : 0;
}
