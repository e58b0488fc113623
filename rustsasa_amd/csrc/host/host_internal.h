// What the host layer's files (radii, reader, prepare, writer, files_mode) share and nobody else sees: views into the
// input text with their inline field parsers, the flat ProtOr table, the `_atom_site` header reader, and the few
// cross-file declarations.  The build has no link-time optimisation: everything called once per character or per atom
// is inline here or stands in the file of the loop that calls it.
#pragma once

#include "../../../include/rustsasa_amd.hpp"

#include <algorithm>
#include <cctype>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace rsasa { const char *tuning_env(const char *name); }  // context.cpp: measurement switches, read only under RSASA_TUNING=1

namespace rustsasa {
namespace detail {

inline std::string trim(const std::string &s)
{
    size_t b = 0, e = s.size();
    while (b < e && std::isspace((unsigned char)s[b])) b++;
    while (e > b && std::isspace((unsigned char)s[e - 1])) e--;
    return s.substr(b, e - b);
}

// ------------------------------------------------------------- text views --

using TextView = std::pair<const char *, size_t>;  // begin and length

// A line of the input text, not copied.
struct LineView {
    const char *p;
    size_t n;
    size_t size() const { return n; }
    const char *data() const { return p; }
    char operator[](size_t i) const { return p[i]; }
    bool starts_with(const char *lit) const
    {
        const size_t k = std::strlen(lit);
        return n >= k && std::memcmp(p, lit, k) == 0;
    }
};

// the next line of `text` from `cur` (advanced past it), without its line end
inline LineView next_line(const char *&cur, const char *end)
{
    const char *nl = (const char *)std::memchr(cur, '\n', (size_t)(end - cur));
    const char *stop = nl ? nl : end;
    LineView line{cur, (size_t)(stop - cur)};
    cur = nl ? nl + 1 : end;
    if (line.n && line.p[line.n - 1] == '\r') line.n--;
    return line;
}

// columns [from, to] (1-based, inclusive) without surrounding white space
inline TextView field_view(const LineView &line, size_t from, size_t to)
{
    if (line.n < from) return {line.p, 0};
    const char *b = line.p + from - 1, *e = line.p + std::min(to, line.n);
    auto space = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };  // isspace in the C locale
    while (b < e && space(*b)) b++;
    while (e > b && space(e[-1])) e--;
    return {b, (size_t)(e - b)};
}

inline bool same(const std::string &s, const TextView &v)
{
    return s.size() == v.second && (v.second == 0 || std::memcmp(s.data(), v.first, v.second) == 0);
}
inline bool same(const TextView &a, const TextView &b) { return a.second == b.second && std::memcmp(a.first, b.first, a.second) == 0; }

// Decimal text -> double.  Plain decimals with at most 15 significant digits (every PDB
// %8.3f field, typical mmCIF Cartn values) take Clinger's exact fast path: an integer below
// 2^53 divided by a power of ten below 10^22 is one correctly rounded IEEE division, so the
// result equals strtod's.  Anything else (exponents, long mantissas, garbage) goes to strtod.
inline double parse_decimal(const char *p, size_t n)
{
    static const double pow10[] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11,
                                   1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    const char *b = p, *e = p + n;
    while (b < e && (*b == ' ' || *b == '\t')) b++;
    while (e > b && (e[-1] == ' ' || e[-1] == '\t')) e--;
    const char *q = b;
    bool neg = false;
    if (q < e && (*q == '-' || *q == '+')) neg = (*q++ == '-');
    unsigned long long mant = 0;
    int digits = 0, frac = 0;
    bool seen_dot = false, ok = q < e;
    for (; q < e; q++) {
        const char c = *q;
        if (c >= '0' && c <= '9') {
            if (mant != 0 || c != '0') digits++;
            mant = mant * 10 + (unsigned)(c - '0');
            if (seen_dot) frac++;
        } else if (c == '.' && !seen_dot) {
            seen_dot = true;
        } else {
            ok = false;
            break;
        }
        if (digits > 15) { ok = false; break; }
    }
    if (ok && frac <= 22) {
        const double v = (double)mant / pow10[frac];
        return neg ? -v : v;
    }
    return std::strtod(std::string(b, (size_t)(e - b)).c_str(), nullptr);
}

// A %w.df field exactly as PDB writers print it - [spaces][-]digits '.' d digits, the point at its column: the same
// integer / power-of-ten division as parse_decimal (so the same double, -0.0 included), without its scanning.  Anything
// else (blank, exponent, shifted point, a sign without digits) returns false and takes the general path.
inline bool fixed_decimal(const char *p, int w, int d, double &out)
{
    static const double pow10[] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6};
    const int dot = w - d - 1;
    if (p[dot] != '.') return false;
    int i = 0;
    while (i < dot && p[i] == ' ') i++;
    bool neg = false;
    if (i < dot && p[i] == '-') { neg = true; i++; }
    if (i == dot) return false;
    unsigned long long mant = 0;
    for (; i < dot; i++) {
        const unsigned c = (unsigned)(p[i] - '0');
        if (c > 9) return false;
        mant = mant * 10 + c;
    }
    for (i = dot + 1; i < w; i++) {
        const unsigned c = (unsigned)(p[i] - '0');
        if (c > 9) return false;
        mant = mant * 10 + c;
    }
    const double v = (double)mant / pow10[d];
    out = neg ? -v : v;
    return true;
}

// columns [from, to] as a decimal; `decimals` > 0: try the fixed %w.df layout first
inline double column_decimal(const LineView &line, size_t from, size_t to, double missing, int decimals = 0)
{
    if (line.size() < from) return missing;
    if (decimals > 0 && line.size() >= to && to - from + 1 <= 12) {
        double v;
        if (fixed_decimal(line.data() + from - 1, (int)(to - from + 1), decimals, v)) return v;
    }
    const size_t len = std::min(to, line.size()) - from + 1;
    const char *p = line.data() + from - 1;
    size_t i = 0;
    while (i < len && p[i] == ' ') i++;
    return i == len ? missing : parse_decimal(p + i, len - i);  // (a blank field is "missing")
}

inline long column_int(const LineView &line, size_t from, size_t to, bool *ok)
{
    long v = 0;
    bool neg = false, any = false, good = true;
    if (line.size() >= from) {
        const size_t end = std::min(to, line.size());
        for (size_t i = from - 1; i < end; i++) {
            const char c = line[i];
            if (c == ' ') { if (any) { for (size_t j = i; j < end; j++) good = good && line[j] == ' '; break; } continue; }
            if (c == '-' && !any && !neg) { neg = true; continue; }
            if (c < '0' || c > '9') { good = false; break; }
            v = v * 10 + (c - '0');
            any = true;
        }
    }
    if (ok) *ok = good && any;
    return neg ? -v : v;
}

// strtol / strtoul on a token: optional sign, then digits up to the first other character
inline long token_long(const TextView &t)
{
    const char *p = t.first, *e = t.first + t.second;
    bool neg = false;
    if (p < e && (*p == '-' || *p == '+')) neg = (*p++ == '-');
    unsigned long v = 0;
    bool over = false;
    for (; p < e && *p >= '0' && *p <= '9'; p++) {
        if (v > (~0ul - 9) / 10) over = true;
        v = v * 10 + (unsigned long)(*p - '0');
    }
    if (over || v > (unsigned long)LONG_MAX) return neg ? LONG_MIN : LONG_MAX;  // strtol saturates
    return neg ? -(long)v : (long)v;
}

// fnv_hash_altloc_serial (utils.rs:83-87 applied to (&str, usize)) on a view: FNV-1a over the str bytes, the 0xff str
// terminator of Rust's Hash impl, then the little-endian usize.  The public function is this body under its other name.
inline std::uint64_t fnv_id(const TextView &alt, std::size_t serial)
{
    std::uint64_t h = 0xcbf29ce484222325ull;
    auto feed = [&h](unsigned char b) { h ^= b; h *= 0x100000001b3ull; };
    for (size_t i = 0; i < alt.second; i++) feed((unsigned char)alt.first[i]);
    feed(0xff);
    std::uint64_t v = (std::uint64_t)serial;
    for (int i = 0; i < 8; i++) feed((unsigned char)(v >> (8 * i)));
    return h;
}

// ------------------------------------------------------------------ radii --

// The ProtOr table as one open-addressing array keyed by the two names packed into 64 bits (residue names of the table
// have at most 3 characters, atom names at most 4): one multiply and usually one probe per atom instead of two string
// hashes.  Names that do not pack (longer) are not in the table.
struct ProtorFlat {
    static constexpr unsigned kBits = 11, kSize = 1u << kBits;  // 2048 slots for about 500 entries
    std::uint64_t key[kSize];
    float radius[kSize];
    static bool pack(const char *res, size_t n_res, const char *atom, size_t n_atom, std::uint64_t *out)
    {
        if (n_res == 0 || n_res > 4 || n_atom == 0 || n_atom > 4) return false;
        std::uint64_t k = 0;
        for (size_t i = 0; i < n_res; i++) k |= (std::uint64_t)(unsigned char)res[i] << (8 * i);
        for (size_t i = 0; i < n_atom; i++) k |= (std::uint64_t)(unsigned char)atom[i] << (32 + 8 * i);
        *out = k;
        return true;
    }
    static unsigned slot(std::uint64_t k) { return (unsigned)((k * 0x9E3779B97F4A7C15ull) >> (64 - kBits)); }
    ProtorFlat();  // radii.cpp, from the embedded table
    bool find(const TextView &res, const TextView &atom, float *out) const
    {
        std::uint64_t k;
        if (!pack(res.first, res.second, atom.first, atom.second, &k)) return false;
        for (unsigned s = slot(k); key[s] != 0; s = (s + 1) & (kSize - 1))
            if (key[s] == k) { *out = radius[s]; return true; }
        return false;
    }
};
const ProtorFlat &protor_flat();

// ---------------------------------------------------------------- readers --

// The readers with their one internal parameter.  Directory mode reads a file, selects its atoms and drops the model:
// unless radii come from the occupancy column nothing ever looks at occupancies or b-factors there, and with
// `skip_occupancy_and_bfactor` two of a record's five decimals are not converted (they keep their defaults, 1.0 and
// 0.0).  The public Structure::from_*_text pass false: full records.
Structure read_pdb_text(const std::string &text, bool skip_occupancy_and_bfactor);
Structure read_mmcif_text(const std::string &text, bool skip_occupancy_and_bfactor);
const std::string &read_whole_file(const std::string &path);  // into a buffer the thread keeps
bool write_whole_file(const std::string &path, const std::string &text, std::string *err);
bool is_mmcif_path(const std::string &path);

// The header of an mmCIF `_atom_site` loop: fed every trimmed, non-empty line, it collects the loop's column names and
// says which lines are the loop's rows; resolve() finds the columns the readers use, once per loop.
struct AtomSiteHeader {
    enum Line { Other, Column, Row };
    std::vector<std::string> cols;
    bool in_loop = false, in_atom_site = false, resolved = false;
    int group = -1, id = -1, sym = -1, atom = -1, alt = -1, comp = -1, lasym = -1, aasym = -1, lseq = -1, aseq = -1,
        ins = -1, x = -1, y = -1, z = -1, occ = -1, b = -1, model = -1;

    Line feed(const LineView &t)
    {
        if (t[0] == 'l' && t.n == 5 && t.starts_with("loop_")) { in_loop = true; in_atom_site = false; cols.clear(); resolved = false; return Other; }
        if (t[0] == '#') { in_loop = false; in_atom_site = false; return Other; }
        if (t[0] == '_') {
            if (!in_loop) return Other;
            in_atom_site = t.starts_with("_atom_site.");
            if (!in_atom_site) return Other;
            const std::string name(t.p + 11, t.n - 11);
            cols.push_back(trim(name.substr(0, name.find_first_of(" \t"))));
            return Column;
        }
        return in_loop && in_atom_site ? Row : Other;
    }
    // before the loop's first row; false: a required column is missing
    bool resolve()
    {
        auto col = [&](const char *name) -> int {
            for (size_t i = 0; i < cols.size(); i++)
                if (cols[i] == name) return (int)i;
            return -1;
        };
        group = col("group_PDB"); id = col("id"); sym = col("type_symbol");
        atom = col("label_atom_id"); alt = col("label_alt_id"); comp = col("label_comp_id");
        lasym = col("label_asym_id"); aasym = col("auth_asym_id"); lseq = col("label_seq_id");
        aseq = col("auth_seq_id"); ins = col("pdbx_PDB_ins_code"); x = col("Cartn_x");
        y = col("Cartn_y"); z = col("Cartn_z"); occ = col("occupancy");
        b = col("B_iso_or_equiv"); model = col("pdbx_PDB_model_num");
        resolved = true;
        return x >= 0 && y >= 0 && z >= 0 && atom >= 0 && comp >= 0;
    }
    // "." and "?" stand for no value
    static TextView value(const TextView &t)
    {
        return (t.second == 1 && (t.first[0] == '.' || t.first[0] == '?')) ? TextView{t.first, 0} : t;
    }
};

// -------------------------------------------------------------- selection --

struct BuildError {
    SASACalcError error = SASACalcError::Ok;
    std::string message;
};

// What one structure contributes to a batch: its kept atoms and the contiguous atom
// segments (residues or chains, by level) whose sequential f32 sums the level reports.
struct Prepared {
    BuildError err;
    std::vector<rsasa_atom_t> atoms;
    std::vector<uint32_t> seg_end;  // end offset (in `atoms`) of each segment, in output order
};

// levels by number, as the test hooks take them: 0 atom, 1 residue, 2 chain, 3 protein
template <typename Level> struct level_index;
template <> struct level_index<AtomLevel> { static constexpr int value = 0; };
template <> struct level_index<ResidueLevel> { static constexpr int value = 1; };
template <> struct level_index<ChainLevel> { static constexpr int value = 2; };
template <> struct level_index<ProteinLevel> { static constexpr int value = 3; };

// build_atoms_and_mapping of each level (options.rs:151-189, 234-286, 317-364, 412-463)
Prepared prepare(const Structure &pdb, const OptionValues &o, int level);

// Directory mode's per-file work, text of one file -> model + Prepared: the short cut when `try_fast` and the file
// qualifies (returns true: `model` then has chains, residues and names but no atoms), else the general reader and
// prepare().  The readers may throw.
bool prepare_text(const std::string &text, bool is_cif, const OptionValues &o, int level, bool try_fast,
                  bool skip_occupancy_and_bfactor, Structure &model, Prepared &prep);

}  // namespace detail
}  // namespace rustsasa
