// Host API, part 2 of 5: the structure model and the general PDB / mmCIF readers (the reference gets its model from
// the pdbtbx crate; this is the library's own minimal one, include/rustsasa_amd.hpp), whole-file reading and writing.
#include "host_internal.h"

#include <cerrno>
#include <cstdio>
#include <fcntl.h>
#include <unistd.h>

namespace rustsasa {

bool Residue::name(std::string *out) const
{
    if (conformers.empty()) return false;
    for (const auto &c : conformers)
        if (c.name != conformers.front().name) return false;
    *out = conformers.front().name;
    return true;
}

std::size_t Structure::atom_count() const
{
    std::size_t n = 0;
    for (const auto &c : chains)
        for (const auto &r : c.residues)
            for (const auto &f : r.conformers) n += f.atoms.size();
    return n;
}

double parse_decimal_text(const std::string &text) { return detail::parse_decimal(text.data(), text.size()); }

// ---- Structure: special members (see the header) ----
Structure::Structure(std::size_t pool_bytes)
    : pool_(new std::pmr::monotonic_buffer_resource(std::max<std::size_t>(pool_bytes, 4096))), chains(pool_.get())
{
}
Structure::Structure(const Structure &other) : chains(other.chains.begin(), other.chains.end()), warnings(other.warnings) {}
Structure::Structure(Structure &&other) noexcept
    : pool_(std::move(other.pool_)), chains(std::move(other.chains)), warnings(std::move(other.warnings))
{
    // the moved-from object must not keep an allocator that points into a pool it no longer owns
    other.chains.~vector();
    new (&other.chains) std::pmr::vector<Chain>();
}
Structure &Structure::operator=(const Structure &other)
{
    if (this != &other) {
        Structure copy(other);
        *this = std::move(copy);
    }
    return *this;
}
Structure &Structure::operator=(Structure &&other) noexcept
{
    if (this != &other) {  // (pmr containers do not take the allocator along on assignment: rebuild in place)
        this->~Structure();
        new (this) Structure(std::move(other));
    }
    return *this;
}

namespace detail {
namespace {

// The model add_atom builds (chains by id, residues by (number, insertion code), conformers by
// (name, alt-loc), existing entries searched from the back), from views into the text: no
// per-line strings, and consecutive atoms of one conformer - nearly all of them - skip the searches.
struct ModelBuilder {
    Structure &s;
    std::pmr::memory_resource *const mem = s.chains.get_allocator().resource();  // the structure's pool
    size_t ci = (size_t)-1, ri = (size_t)-1, fi = (size_t)-1;  // chain / residue / conformer of the previous atom

    // a new, default-constructed record at the end of the atom's conformer
    AtomRecord &add(const TextView &chain_id, std::int64_t res_seq, const TextView &icode, const TextView &res_name,
                    const TextView &alt, size_t expect = 16)
    {
        if (ci == (size_t)-1 || !same(s.chains[ci].id, chain_id)) {
            ci = (size_t)-1;
            for (size_t k = s.chains.size(); k-- > 0;)
                if (same(s.chains[k].id, chain_id)) { ci = k; break; }
            if (ci == (size_t)-1) {
                s.chains.push_back(Chain{std::string(chain_id.first, chain_id.second), std::pmr::vector<Residue>(mem)});
                ci = s.chains.size() - 1;
            }
            ri = fi = (size_t)-1;
        }
        Chain &chain = s.chains[ci];
        if (ri == (size_t)-1 || chain.residues[ri].serial_number != res_seq || !same(chain.residues[ri].insertion_code, icode)) {
            ri = (size_t)-1;
            for (size_t k = chain.residues.size(); k-- > 0;)
                if (chain.residues[k].serial_number == res_seq && same(chain.residues[k].insertion_code, icode)) { ri = k; break; }
            if (ri == (size_t)-1) {
                chain.residues.push_back(Residue{res_seq, std::string(icode.first, icode.second), std::pmr::vector<Conformer>(mem)});
                ri = chain.residues.size() - 1;
            }
            fi = (size_t)-1;
        }
        Residue &res = chain.residues[ri];
        if (fi == (size_t)-1 || !same(res.conformers[fi].name, res_name) || !same(res.conformers[fi].alt_loc, alt)) {
            fi = (size_t)-1;
            for (size_t k = 0; k < res.conformers.size(); k++)
                if (same(res.conformers[k].name, res_name) && same(res.conformers[k].alt_loc, alt)) { fi = k; break; }
            if (fi == (size_t)-1) {
                res.conformers.push_back(Conformer{std::string(res_name.first, res_name.second), std::string(alt.first, alt.second),
                                                   std::pmr::vector<AtomRecord>(mem)});
                fi = res.conformers.size() - 1;
            }
        }
        std::pmr::vector<AtomRecord> &atoms = res.conformers[fi].atoms;
        if (atoms.capacity() == atoms.size()) atoms.reserve(std::max<size_t>(expect, 2 * atoms.size()));
        atoms.emplace_back();
        last_atoms = &atoms;
        return atoms.back();
    }
    // one more record in the conformer of the previous add() (the caller knows that chain, residue, conformer are the
    // same: a run of records with identical columns 17-27); no searches, no comparisons
    std::pmr::vector<AtomRecord> *last_atoms = nullptr;
    AtomRecord &add_to_last()
    {
        last_atoms->emplace_back();
        return last_atoms->back();
    }
};

// the symbol in upper case, else the first letter of the name
inline void set_element(AtomRecord &rec, const TextView &symbol)
{
    rec.element.assign(symbol.first, symbol.second);
    for (auto &c : rec.element) c = (char)std::toupper((unsigned char)c);
    if (!rec.element.empty()) return;
    for (unsigned char c : rec.name)
        if (std::isalpha(c)) { rec.element.assign(1, (char)std::toupper(c)); return; }
}

// Atoms without an alternate location belong to EVERY conformer of a residue that has alternate locations
// (a side chain modelled twice on one backbone): the blank conformer's atoms are appended to each of the
// others and the blank conformer goes.  The reference's `residue.conformers().next()` (src/options.rs:162,255)
// then selects backbone + first alternate location, which is what its quality gate over the FreeSASA set
// (tests/quality.rs:17-18, RMSE 43.99 of the reference itself) implies for pdbtbx - whose source is not in
// the reference tree, so the order inside a conformer (its own atoms, then the shared ones) is our choice.
inline void share_blank_conformers(Structure &s)
{
    for (Chain &chain : s.chains)
        for (Residue &res : chain.residues) {
            if (res.conformers.size() < 2) continue;
            size_t blank = res.conformers.size();
            for (size_t k = 0; k < res.conformers.size(); k++)
                if (res.conformers[k].alt_loc.empty()) { blank = k; break; }
            if (blank == res.conformers.size()) continue;
            const Conformer shared = std::move(res.conformers[blank]);
            res.conformers.erase(res.conformers.begin() + (std::ptrdiff_t)blank);
            for (Conformer &c : res.conformers) c.atoms.insert(c.atoms.end(), shared.atoms.begin(), shared.atoms.end());
        }
}

// A pool for the model of `text_bytes` of PDB / mmCIF text: an atom record takes 1.5 bytes per byte of an 80-column
// line, residues and conformers a little more.
inline std::size_t pool_bytes_for(std::size_t text_bytes) { return text_bytes * 2 + 4096; }

// mmCIF tokens of one row as views: white-space separated, '...' and "..." quoting (a quote ends
// at the quote character that is followed by white space or the end of the line).
inline void tokenize_views(const LineView &line, std::vector<TextView> &out)
{
    out.clear();
    auto space = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    size_t i = 0;
    const size_t n = line.n;
    const char *p = line.p;
    while (i < n) {
        while (i < n && space(p[i])) i++;
        if (i >= n) break;
        if (p[i] == '\'' || p[i] == '"') {
            const char q = p[i++];
            size_t j = i;
            while (j < n && !(p[j] == q && (j + 1 == n || space(p[j + 1])))) j++;
            out.push_back({p + i, j - i});
            i = j + 1;
        } else {
            size_t j = i;
            while (j < n && !space(p[j])) j++;
            out.push_back({p + i, j - i});
            i = j;
        }
    }
}

}  // namespace

Structure read_pdb_text(const std::string &text, bool skip_occupancy_and_bfactor)
{
    Structure s(pool_bytes_for(text.size()));
    ModelBuilder model{s};
    bool in_first_model = true, seen_model = false;
    std::size_t counter = 0, run_left = 0, run_len = 1;
    const char *cur = text.data(), *const end = text.data() + text.size();
    while (cur < end) {
        const LineView line = next_line(cur, end);
        if (line.starts_with("MODEL")) {
            if (seen_model) in_first_model = false;
            seen_model = true;
            continue;
        }
        if (line.starts_with("ENDMDL")) { in_first_model = false; continue; }
        const bool is_atom = line.starts_with("ATOM  "), is_het = line.starts_with("HETATM");
        if (!(is_atom || is_het) || !in_first_model) continue;
        if (line.n < 54) { s.warnings.push_back("short ATOM record skipped"); continue; }
        counter++;
        // records of one conformer usually follow each other: count them (columns 17-27: alternate location, residue
        // name, chain, number, insertion code) so that the conformer's atoms are allocated once, at their final size
        if (run_left == 0) {
            run_left = 1;
            if (line.n >= 27) {
                const char *scan = cur;
                while (scan < end) {
                    const LineView nl = next_line(scan, end);
                    if (nl.starts_with("ANISOU")) continue;  // (between an atom and the next one)
                    if (nl.n < 54 || !(nl.starts_with("ATOM  ") || nl.starts_with("HETATM")) || std::memcmp(nl.p + 16, line.p + 16, 11) != 0) break;
                    run_left++;
                }
            }
            run_len = run_left;
        }
        const bool run_start = run_left == run_len;
        run_left--;
        const TextView name = field_view(line, 13, 16);
        // (the records of a run share columns 17-27: only its first one looks its conformer up)
        AtomRecord &rec = run_start ? model.add(field_view(line, 22, 22), column_int(line, 23, 26, nullptr), field_view(line, 27, 27),
                                                field_view(line, 18, 20), field_view(line, 17, 17), run_len)
                                    : model.add_to_last();
        rec.hetero = is_het;
        bool serial_ok = false;
        const long sv = column_int(line, 7, 11, &serial_ok);
        rec.serial = serial_ok ? (std::size_t)sv : counter;
        rec.name.assign(name.first, name.second);
        rec.x = column_decimal(line, 31, 38, 0.0, 3);  // %8.3f
        rec.y = column_decimal(line, 39, 46, 0.0, 3);
        rec.z = column_decimal(line, 47, 54, 0.0, 3);
        if (!skip_occupancy_and_bfactor) {
            rec.occupancy = column_decimal(line, 55, 60, 1.0, 2);  // %6.2f
            rec.b_factor = column_decimal(line, 61, 66, 0.0, 2);
        }
        set_element(rec, field_view(line, 77, 78));
    }
    share_blank_conformers(s);
    return s;
}

Structure read_mmcif_text(const std::string &text, bool skip_occupancy_and_bfactor)
{
    Structure s(pool_bytes_for(text.size()));
    ModelBuilder model{s};
    AtomSiteHeader h;
    std::vector<TextView> tok;
    std::string first_model;
    auto val = [&](int c) -> TextView {
        return c < 0 || c >= (int)tok.size() ? TextView{"", 0} : AtomSiteHeader::value(tok[c]);
    };
    const char *cur = text.data(), *const end = text.data() + text.size();
    while (cur < end) {
        const LineView raw = next_line(cur, end);
        const TextView tv = field_view(raw, 1, raw.n);  // trimmed
        if (tv.second == 0 || h.feed({tv.first, tv.second}) != AtomSiteHeader::Row) continue;
        if (!h.resolved && !h.resolve()) throw std::runtime_error("mmCIF _atom_site loop lacks required columns");
        tokenize_views({tv.first, tv.second}, tok);
        if (tok.size() < h.cols.size()) { s.warnings.push_back("short _atom_site row skipped"); continue; }  // (long rows pass)
        const TextView model_id = val(h.model);
        if (first_model.empty()) first_model = model_id.second ? std::string(model_id.first, model_id.second) : "1";
        if (model_id.second && !same(first_model, model_id)) continue;
        const TextView chain_id = val(h.aasym).second ? val(h.aasym) : val(h.lasym);
        const TextView seq = val(h.aseq).second ? val(h.aseq) : val(h.lseq);
        const TextView name = val(h.atom), group = val(h.group);
        AtomRecord &rec = model.add(chain_id, token_long(seq), val(h.ins), val(h.comp), val(h.alt));
        rec.hetero = group.second == 6 && std::memcmp(group.first, "HETATM", 6) == 0;
        rec.serial = (std::size_t)token_long(val(h.id));
        rec.name.assign(name.first, name.second);
        auto num = [&](int c, double missing) {
            const TextView v = val(c);
            return v.second ? parse_decimal(v.first, v.second) : missing;
        };
        rec.x = num(h.x, 0.0);
        rec.y = num(h.y, 0.0);
        rec.z = num(h.z, 0.0);
        if (!skip_occupancy_and_bfactor) {
            rec.occupancy = num(h.occ, 1.0);
            rec.b_factor = num(h.b, 0.0);
        }
        set_element(rec, val(h.sym));
    }
    share_blank_conformers(s);
    return s;
}

const std::string &read_whole_file(const std::string &path)
{
    static thread_local std::string text;  // (no stream, no copies of the text)
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    text.clear();
    if (std::fseek(f, 0, SEEK_END) == 0) {
        const long size = std::ftell(f);
        if (size > 0) text.resize((size_t)size);
        std::rewind(f);
    }
    size_t got = 0;
    for (;;) {
        if (got == text.size()) text.resize(std::max<size_t>(2 * text.size(), 1 << 16));  // unknown or growing size
        const size_t n = std::fread(&text[got], 1, text.size() - got, f);
        got += n;
        if (n == 0) break;
    }
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) throw std::runtime_error("cannot read " + path);
    text.resize(got);
    return text;
}

// fs::write: create or truncate, write all, close (POSIX; short writes continued)
bool write_whole_file(const std::string &path, const std::string &text, std::string *err)
{
    auto fail = [&] { *err = "cannot write " + path + ": " + std::strerror(errno); return false; };
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) return fail();
    size_t done = 0;
    while (done < text.size()) {
        const ssize_t n = ::write(fd, text.data() + done, text.size() - done);
        if (n < 0) {
            if (errno == EINTR) continue;
            fail();
            ::close(fd);
            return false;
        }
        done += (size_t)n;
    }
    return ::close(fd) == 0 || fail();
}

bool is_mmcif_path(const std::string &path)
{
    const size_t dot = path.find_last_of('.');
    std::string ext = dot == std::string::npos ? std::string() : path.substr(dot);
    for (auto &c : ext) c = (char)std::toupper((unsigned char)c);
    return ext == ".CIF" || ext == ".MMCIF";
}

}  // namespace detail

Structure Structure::from_pdb_text(const std::string &text) { return detail::read_pdb_text(text, false); }
Structure Structure::from_mmcif_text(const std::string &text) { return detail::read_mmcif_text(text, false); }

Structure Structure::open(const std::string &path)
{
    const std::string &text = detail::read_whole_file(path);
    return detail::is_mmcif_path(path) ? from_mmcif_text(text) : from_pdb_text(text);
}

}  // namespace rustsasa
