// gol_cli.cpp -- the reference program's surface on top of libgol.so.
//
// Mirrors main() of Parallel_Life_MPI.cpp:190-240:
//   * reads `h w epochs` from grid_size_data.txt (:201-209) and the h lines of
//     data.txt (:56-102) from the working directory (or --dir);
//   * advances `epochs` generations on the GPU (:215-221);
//   * writes output.txt (:147-188) without truncating it (the reference opens it
//     with MPI_MODE_WRONLY|MPI_MODE_CREATE, :170), at the same offsets;
//   * prints "Process r wrote data to the file." per rank (:179) and
//     "Total time = X" (:236), X being wall seconds including I/O (:199, :233).
//
// --ref-ranks P reproduces `mpirun -np P` byte for byte (GOL_SEM_REF_STRIPES:
// the reference's halo exchange is a no-op, so its output depends on P).
// Without it the field evolves as one domain (== the reference at -np 1).
// --gpus G splits that domain into G row stripes on devices 0..G-1 of this
// process with k-deep halo rounds over xGMI peer copies (gol_create_group);
// --stripes S runs S stripes round-robin on the G devices (S >= G).
// --torus joins the field's opposite edges (GOL_SEM_TORUS): same files, same
// output.txt format; one engine on one GPU, so not with --ref-ranks, nor with
// --gpus or --stripes above 1.  --halo-depth then sets the generations per wrap
// round.
// --paste FILE@Y,X[:set|or|xor|clear] combines the cells of FILE (data.txt format:
// lines of '0'/'1', its height and width are those of its lines) into the field
// with its first cell at row Y, column X (gol_write_rect; default set).  Repeatable,
// applied in order after data.txt is loaded and before the first generation.
// --window Y,X,H,W writes only that window to output.txt (gol_read_rect): H lines of
// W cells; the file is truncated to them.  With --torus either may cross the seams.
// --until-periodic LAG[:EVERY] runs the epochs with gol_step_until_periodic(epochs, LAG,
// EVERY, GOL_UNTIL_FINISH): once generation g's field equals generation g - LAG's the
// remaining generations are reduced modulo the period, so output.txt holds the bytes
// the run without the flag writes; one extra line reports g and the period, or that
// none was found.  One engine only: not with --ref-ranks, --gpus or --stripes.
//
// Deviation: where the reference prints an error and continues with
// uninitialised values (:206) or an unopened file (:186), this program exits
// with status 1.
#include <fcntl.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/gol.h"

namespace {

bool parse_rule(const std::string& s, uint32_t* b, uint32_t* sv)
{
    if (s == "ref") {
        *b = GOL_REF_BIRTH;
        *sv = GOL_REF_SURVIVE;
        return true;
    }
    if (s == "conway") {
        *b = GOL_CONWAY_BIRTH;
        *sv = GOL_CONWAY_SURVIVE;
        return true;
    }
    // "B<digits>/S<digits>"
    if (s.size() < 3 || (s[0] != 'B' && s[0] != 'b')) return false;
    size_t slash = s.find('/');
    if (slash == std::string::npos || slash + 1 >= s.size() ||
        (s[slash + 1] != 'S' && s[slash + 1] != 's'))
        return false;
    uint32_t bm = 0, sm = 0;
    for (size_t i = 1; i < slash; ++i) {
        if (s[i] < '0' || s[i] > '8') return false;
        bm |= 1u << (s[i] - '0');
    }
    for (size_t i = slash + 2; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '8') return false;
        sm |= 1u << (s[i] - '0');
    }
    *b = bm;
    *sv = sm;
    return true;
}

void usage()
{
    std::cerr << "usage: gol [--dir DIR] [--ref-ranks P] [--rule ref|conway|B3/S23]\n"
                 "           [--tb-depth K] [--rows-per-wave N] [--device D]\n"
                 "           [--gpus G] [--stripes S] [--halo-depth H] [--torus]\n"
                 "           [--paste FILE@Y,X[:set|or|xor|clear]]... [--window Y,X,H,W]\n"
                 "           [--until-periodic LAG[:EVERY]]\n"
                 "Reads grid_size_data.txt and data.txt, writes output.txt.\n"
                 "--paste: combine the cells of FILE (lines of 0/1) into the loaded field at\n"
                 "         row Y, column X before stepping (default set); repeatable.\n"
                 "--window: output.txt holds only the H x W window at row Y, column X.\n"
                 "--until-periodic: stop computing once the field repeats with a period that\n"
                 "         divides LAG (checked every EVERY generations, default the next\n"
                 "         multiple of 64); output.txt is the same.  Not with --ref-ranks,\n"
                 "         --gpus or --stripes.\n"
                 "--torus: the field's opposite edges are joined (periodic boundary);\n"
                 "         not with --ref-ranks, nor with --gpus / --stripes above 1.\n";
}

bool read_file(const std::string& path, size_t need, std::vector<char>& out)
{
    int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    out.resize(need);
    size_t got = 0;
    while (got < need) {
        ssize_t n = ::pread(fd, out.data() + got, need - got, (off_t)got);
        if (n <= 0) break;
        got += (size_t)n;
    }
    ::close(fd);
    return got == need;
}

// --paste FILE@Y,X[:op]
struct Paste {
    std::string file;
    uint64_t y = 0, x = 0, h = 0, w = 0;
    uint32_t op = GOL_RECT_SET;
    std::vector<uint64_t> words;  // packed, ceil(w/64) per row
};

bool parse_u64s(const std::string& s, uint64_t* v, int n)
{
    const char* p = s.c_str();
    for (int i = 0; i < n; ++i) {
        if (*p < '0' || *p > '9') return false;
        char* end = nullptr;
        v[i] = std::strtoull(p, &end, 10);
        p = end;
        if (i + 1 < n) {
            if (*p != ',') return false;
            ++p;
        }
    }
    return *p == 0;
}

bool parse_paste(const std::string& a, Paste* out)
{
    const size_t at = a.rfind('@');
    if (at == std::string::npos || at == 0) return false;
    out->file = a.substr(0, at);
    std::string pos = a.substr(at + 1);
    const size_t colon = pos.find(':');
    if (colon != std::string::npos) {
        const std::string op = pos.substr(colon + 1);
        if (op == "set") out->op = GOL_RECT_SET;
        else if (op == "or") out->op = GOL_RECT_OR;
        else if (op == "xor") out->op = GOL_RECT_XOR;
        else if (op == "clear") out->op = GOL_RECT_CLEAR;
        else return false;
        pos = pos.substr(0, colon);
    }
    uint64_t v[2];
    if (!parse_u64s(pos, v, 2)) return false;
    out->y = v[0];
    out->x = v[1];
    return true;
}

// Reads a paste file: equal lines of '0' / '1', each ended by '\n' (the last one may
// lack it).  Returns an error message, empty on success.
std::string load_paste(Paste* p)
{
    std::ifstream f(p->file, std::ios::binary);
    if (!f) return "cannot open";
    const std::string txt((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    while (pos < txt.size()) {
        size_t nl = txt.find('\n', pos);
        if (nl == std::string::npos) nl = txt.size();
        const uint64_t len = nl - pos;
        if (p->h == 0) p->w = len;
        if (len != p->w || len == 0) return "lines of unequal or zero length";
        const uint64_t wq = (p->w + 63) / 64;
        p->words.resize((size_t)((p->h + 1) * wq), 0);
        for (uint64_t j = 0; j < len; ++j) {
            const char c = txt[pos + j];
            if (c != '0' && c != '1') return "a byte other than '0' or '1'";
            if (c == '1') p->words[(size_t)(p->h * wq + j / 64)] |= 1ull << (j & 63);
        }
        ++p->h;
        pos = nl + 1;
    }
    return p->h ? "" : "empty file";
}

}  // namespace

int main(int argc, char** argv)
{
    const auto t0 = std::chrono::steady_clock::now();  // MPI_Wtime() at :199
    std::string dir = ".";
    int gpus = 0, stripes = 0;
    bool torus = false, ref_ranks = false, window = false, until = false;
    uint64_t lag_every[2] = {0, 0};  // --until-periodic LAG[:EVERY]
    uint64_t win[4] = {0, 0, 0, 0};  // Y, X, H, W
    std::vector<Paste> pastes;
    gol_config cfg;
    gol_config_init(&cfg);
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string {
            if (i + 1 >= argc) {
                usage();
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--dir") dir = next();
        else if (a == "--ref-ranks") {
            cfg.ref_ranks = (uint32_t)std::strtoul(next().c_str(), nullptr, 10);
            cfg.semantics = GOL_SEM_REF_STRIPES;
            ref_ranks = true;
        } else if (a == "--torus") torus = true;
        else if (a == "--rule") {
            if (!parse_rule(next(), &cfg.birth_mask, &cfg.survive_mask)) {
                std::cerr << "bad rule\n";
                return 2;
            }
        } else if (a == "--tb-depth") cfg.tb_depth = (uint32_t)std::strtoul(next().c_str(), nullptr, 10);
        else if (a == "--rows-per-wave") cfg.rows_per_wave = (uint32_t)std::strtoul(next().c_str(), nullptr, 10);
        else if (a == "--device") cfg.device = (int32_t)std::strtol(next().c_str(), nullptr, 10);
        else if (a == "--gpus") gpus = (int)std::strtol(next().c_str(), nullptr, 10);
        else if (a == "--stripes") stripes = (int)std::strtol(next().c_str(), nullptr, 10);
        else if (a == "--halo-depth") cfg.halo_depth = (uint32_t)std::strtoul(next().c_str(), nullptr, 10);
        else if (a == "--paste") {
            Paste p;
            if (!parse_paste(next(), &p)) {
                std::cerr << "bad --paste, want FILE@Y,X[:set|or|xor|clear]\n";
                return 2;
            }
            pastes.push_back(p);
        } else if (a == "--window") {
            if (!parse_u64s(next(), win, 4)) {
                std::cerr << "bad --window, want Y,X,H,W\n";
                return 2;
            }
            window = true;
        } else if (a == "--until-periodic") {
            std::string v = next();
            const size_t colon = v.find(':');
            const bool ok = colon == std::string::npos
                                ? parse_u64s(v, lag_every, 1)
                                : parse_u64s(v.substr(0, colon), lag_every, 1) &&
                                      parse_u64s(v.substr(colon + 1), lag_every + 1, 1);
            if (!ok || lag_every[0] > UINT32_MAX || lag_every[1] > UINT32_MAX) {
                std::cerr << "bad --until-periodic, want LAG[:EVERY]\n";
                return 2;
            }
            until = true;
        } else if (a == "-h" || a == "--help") {
            usage();
            return 0;
        } else {
            usage();
            return 2;
        }
    }

    if (torus) {
        if (ref_ranks || gpus > 1 || stripes > 1) {
            std::cerr << "--torus is one field on one GPU; drop --ref-ranks, --gpus and --stripes"
                      << std::endl;
            return 2;
        }
        cfg.semantics = GOL_SEM_TORUS;
        gpus = stripes = 0;  // (--gpus 1 / --stripes 1: the one engine below)
    }

    if (until && (ref_ranks || gpus > 0 || stripes > 0)) {
        std::cerr << "--until-periodic needs the one engine of one field; drop --ref-ranks, --gpus "
                     "and --stripes"
                  << std::endl;
        return 2;
    }

    long long h = 0, w = 0, epochs = 0;
    {
        std::ifstream gs(dir + "/grid_size_data.txt");
        if (!(gs >> h >> w >> epochs)) {
            std::cerr << "Error reading integers from file." << std::endl;  // :206
            return 1;
        }
    }
    if (h <= 0 || w <= 0 || epochs < 0) {
        std::cerr << "Invalid grid size or epoch count." << std::endl;
        return 1;
    }
    const uint32_t P = cfg.semantics == GOL_SEM_REF_STRIPES ? cfg.ref_ranks : 1;
    if (P == 0 || (uint64_t)h / P == 0) {
        std::cerr << "Need 1 <= ranks <= rows." << std::endl;
        return 1;
    }
    const size_t bytes = (size_t)h * (size_t)(w + 1);
    std::vector<char> data;
    if (!read_file(dir + "/data.txt", bytes, data)) {
        std::cerr << "Error reading data.txt (need " << bytes << " bytes)." << std::endl;
        return 1;
    }

    for (auto& p : pastes) {
        const std::string err = load_paste(&p);
        if (!err.empty()) {
            std::cerr << "gol error " << (int)GOL_EINVAL << ": paste file " << p.file << ": " << err
                      << std::endl;
            return 1;
        }
    }
    // region I/O on the engines of either path below (a group: every member takes
    // its own rows; the members' windows are OR-ed)
    auto paste_all = [&](const std::vector<gol_engine*>& es) {
        for (const auto& p : pastes)
            for (auto* e : es) {
                const gol_status st = gol_write_rect(e, p.y, p.x, p.h, p.w, p.words.data(),
                                                     (p.w + 63) / 64, p.op);
                if (st != GOL_OK) return st;
            }
        return GOL_OK;
    };
    auto read_window = [&](const std::vector<gol_engine*>& es, std::vector<char>& txt) {
        const uint64_t ww = (win[3] + 63) / 64;
        std::vector<uint64_t> acc((size_t)(win[2] * ww), 0), one(acc.size(), 0);
        for (auto* e : es) {
            const gol_status st = gol_read_rect(e, win[0], win[1], win[2], win[3], one.data(), ww);
            if (st != GOL_OK) return st;
            for (size_t i = 0; i < acc.size(); ++i) acc[i] |= one[i];
        }
        txt.assign((size_t)(win[2] * (win[3] + 1)), '\n');
        for (uint64_t i = 0; i < win[2]; ++i)
            for (uint64_t j = 0; j < win[3]; ++j)
                txt[(size_t)(i * (win[3] + 1) + j)] =
                    ((acc[(size_t)(i * ww + j / 64)] >> (j & 63)) & 1) ? '1' : '0';
        return GOL_OK;
    };
    const bool edits = !pastes.empty() || window;

    std::vector<char> out(bytes);
    if (gpus > 0 || stripes > 0) {
        if (cfg.semantics != GOL_SEM_GLOBAL) {
            std::cerr << "--gpus/--stripes evolve one global field; drop --ref-ranks" << std::endl;
            return 1;
        }
        if (gpus <= 0) gpus = 1;
        if (stripes <= 0) stripes = gpus;
        if ((uint64_t)h / (uint64_t)stripes == 0) {
            std::cerr << "Need 1 <= stripes <= rows." << std::endl;
            return 1;
        }
    }
    gol_until found{};
    found.struct_size = sizeof(gol_until);
    if (epochs == 0 && !edits && !until) {
        // zero generations: the reference writes the input bytes back (:157-164)
        out = data;
    } else if (stripes > 0) {
        std::vector<gol_engine*> es((size_t)stripes, nullptr);
        std::vector<int> devs((size_t)stripes);
        for (int r = 0; r < stripes; ++r) devs[(size_t)r] = r % gpus;
        gol_status st = gol_create_group((uint64_t)h, (uint64_t)w, &cfg, stripes, devs.data(),
                                         es.data());
        for (int r = 0; r < stripes && st == GOL_OK; ++r) {
            uint64_t r0 = 0, n = 0;
            gol_rank_rows((uint64_t)h, stripes, r, &r0, &n);
            st = gol_load_ascii(es[(size_t)r], data.data() + r0 * (uint64_t)(w + 1),
                                n * (uint64_t)(w + 1));
        }
        if (st == GOL_OK) st = paste_all(es);
        if (st == GOL_OK && epochs > 0) st = gol_group_step(es.data(), stripes, (uint64_t)epochs);
        if (st == GOL_OK && window) st = read_window(es, out);
        for (int r = 0; r < stripes && st == GOL_OK && !window; ++r) {
            uint64_t r0 = 0, n = 0;
            gol_rank_rows((uint64_t)h, stripes, r, &r0, &n);
            st = gol_store_ascii(es[(size_t)r], out.data() + r0 * (uint64_t)(w + 1),
                                 n * (uint64_t)(w + 1));
        }
        if (st != GOL_OK) std::cerr << "gol error " << (int)st << ": " << gol_last_error() << std::endl;
        for (auto* e : es) gol_destroy(e);
        if (st != GOL_OK) return 1;
    } else {
        gol_engine* e = nullptr;
        gol_status st = gol_create((uint64_t)h, (uint64_t)w, &cfg, &e);
        if (st == GOL_OK) st = gol_load_ascii(e, data.data(), data.size());
        if (st == GOL_OK) st = paste_all({e});
        if (st == GOL_OK && until)
            st = gol_step_until_periodic(e, (uint64_t)epochs, (uint32_t)lag_every[0],
                                         (uint32_t)lag_every[1], GOL_UNTIL_FINISH, &found);
        else if (st == GOL_OK && epochs > 0)
            st = gol_step(e, (uint64_t)epochs);
        if (st == GOL_OK) st = gol_sync(e);
        if (st == GOL_OK) st = window ? read_window({e}, out) : gol_store_ascii(e, out.data(), out.size());
        if (st != GOL_OK) {
            std::cerr << "gol error " << (int)st << ": " << gol_last_error() << std::endl;
            gol_destroy(e);
            return 1;
        }
        gol_destroy(e);
    }

    if (until) {
        if (found.period)
            std::cout << "Period " << found.period << " from generation " << found.advanced
                      << " on (lag " << found.lag << ", checked every " << found.check_every
                      << " generations)." << std::endl;
        else
            std::cout << "No period dividing " << found.lag << " within " << epochs
                      << " generations (checked every " << found.check_every << ")." << std::endl;
    }

    // writeDataToFile (:166-183): create if missing, never truncate, each rank's
    // rows at r*(h/P)*(w+1); together they cover [0, h*(w+1)).
    int fd = ::open((dir + "/output.txt").c_str(), O_WRONLY | O_CREAT, 0666);
    if (fd < 0) {
        std::cerr << "Error opening the file for writing." << std::endl;  // :186
        return 1;
    }
    // (--window: the file holds the window alone, written by "rank" 0)
    if (window && ::ftruncate(fd, 0) != 0) {
        std::cerr << "Error writing output.txt." << std::endl;
        ::close(fd);
        return 1;
    }
    const uint32_t writers = window ? 1 : P;
    const size_t total = window ? out.size() : bytes;
    const size_t chunk = window ? total : (size_t)(h / P) * (size_t)(w + 1);
    for (uint32_t r = 0; r < writers; ++r) {
        const size_t off = (size_t)r * chunk;
        const size_t len = (r == writers - 1) ? total - off : chunk;
        size_t done = 0;
        while (done < len) {
            ssize_t n = ::pwrite(fd, out.data() + off + done, len - done, (off_t)(off + done));
            if (n <= 0) {
                std::cerr << "Error writing output.txt." << std::endl;
                ::close(fd);
                return 1;
            }
            done += (size_t)n;
        }
        std::cout << "Process " << r << " wrote data to the file." << std::endl;  // :179
    }
    ::close(fd);

    const double secs =
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "Total time = " << secs << std::endl;  // :236
    return 0;
}
