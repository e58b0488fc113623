// Host API, part 4 of 5: from a structure, or straight from a file's text, to what the GPU is handed - the kept atoms
// (first conformer per residue, hydrogen / HETATM filters, radii by options) and the segment ends of the level.
#include "host_internal.h"

#include <chrono>
#include <cstdio>
#include <string_view>

#if defined(__SSE2__) && !defined(__HIP_DEVICE_COMPILE__)
#include <emmintrin.h>  // (the mmCIF short cut finds a row's separators sixteen bytes at a time)

#define RSASA_ROW_SSE2 1
#endif

namespace rustsasa {
namespace detail {

namespace {

// build_atom! (options.rs:81-116)
bool build_atom(const OptionValues &o, const AtomRecord &atom, const std::string &residue_name,
                std::uint64_t id, std::vector<rsasa_atom_t> &atoms, BuildError &err)
{
    float radius = 0.f;
    if (o.read_radii_from_occupancy) {
        radius = (float)atom.occupancy;
    } else {
        bool found = false;
        if (o.radii_config) {  // utils.rs:45-53
            auto r = o.radii_config->find(residue_name);
            if (r != o.radii_config->end()) {
                auto a = r->second.find(atom.name);
                if (a != r->second.end()) { radius = a->second; found = true; }
            }
        }
        if (!found) found = get_protor_radius(residue_name, atom.name, &radius);
        if (!found) {
            if (o.allow_vdw_fallback) {
                if (!vdw_radius(atom.element, &radius)) {
                    err = {SASACalcError::VanDerWaalsMissing, "Van der Waals radius missing for element"};
                    return false;
                }
            } else {
                err = {SASACalcError::RadiusMissing,
                       "Radius not found for residue '" + residue_name + "' atom '" + atom.name +
                           "' of type '" + atom.element +
                           "'. This error can can be ignored, if you are using the CLI pass "
                           "--allow-vdw-fallback or use with_allow_vdw_fallback if you are using the API."};
                return false;
            }
        }
    }
    rsasa_atom_t a;
    a.position[0] = (float)atom.x;  // options.rs:106-110: f64 -> f32
    a.position[1] = (float)atom.y;
    a.position[2] = (float)atom.z;
    a.radius = radius;
    a.id = id;
    atoms.push_back(a);
    return true;
}

// The atom loop shared by all four build_atoms_and_mapping bodies: chains ->
// residues -> FIRST conformer -> atoms, hydrogen / HETATM filters.  `per_residue`
// is told each residue's range of kept atoms.
template <typename F>
bool select_atoms(const Structure &pdb, const OptionValues &o, bool id_uses_altloc,
                  std::vector<rsasa_atom_t> &atoms, BuildError &err, F per_residue)
{
    atoms.reserve(atoms.size() + pdb.atom_count());  // (an upper bound: one allocation instead of a dozen regrowths)
    for (size_t ci = 0; ci < pdb.chains.size(); ci++) {
        const Chain &chain = pdb.chains[ci];
        for (size_t ri = 0; ri < chain.residues.size(); ri++) {
            const Residue &res = chain.residues[ri];
            // Residue::name(): Some(name) iff every conformer has the same name (options.rs:161,248); no copy
            bool same_name = !res.conformers.empty();
            for (size_t k = 1; k < res.conformers.size() && same_name; k++) same_name = res.conformers[k].name == res.conformers[0].name;
            if (!same_name) {
                err = {SASACalcError::FailedToGetResidueName, "Failed to get residue name"};
                return false;
            }
            const Conformer &conf = res.conformers.front();  // conformers().next()
            const TextView alt{conf.alt_loc.data(), id_uses_altloc ? conf.alt_loc.size() : 0};
            const size_t begin = atoms.size();
            for (const AtomRecord &atom : conf.atoms) {
                if (atom.element.empty()) {  // options.rs:164
                    err = {SASACalcError::ElementMissing, "Element missing for atom"};
                    return false;
                }
                if (!o.include_hydrogens && atom.element.size() == 1 && atom.element[0] == 'H') continue;  // options.rs:166
                if (atom.hetero && !o.include_hetatms) continue;           // options.rs:169
                if (!build_atom(o, atom, conf.name, fnv_id(alt, atom.serial), atoms, err)) return false;
            }
            per_residue(ci, begin, atoms.size());
        }
    }
    return true;
}

}  // namespace

Prepared prepare(const Structure &pdb, const OptionValues &o, int level)
{
    Prepared p;
    if (level == level_index<ChainLevel>::value) {
        std::vector<uint32_t> chain_end(pdb.chains.size(), 0u);
        select_atoms(pdb, o, true, p.atoms, p.err, [&](size_t ci, size_t, size_t end) { chain_end[ci] = (uint32_t)end; });
        // kept atoms of a chain are contiguous; a chain without residues owns an empty range
        uint32_t prev = 0;
        for (size_t ci = 0; ci < pdb.chains.size(); ci++) {
            prev = std::max(prev, chain_end[ci]);
            p.seg_end.push_back(prev);
        }
    } else {  // residue ends, none at atom level; ProteinLevel's ids ignore the alt-loc (options.rs:453)
        const bool segments = level != level_index<AtomLevel>::value;
        select_atoms(pdb, o, level != level_index<ProteinLevel>::value, p.atoms, p.err,
                     [&](size_t, size_t, size_t end) { if (segments) p.seg_end.push_back((uint32_t)end); });
    }
    return p;
}

namespace {

// ---- directory mode's short cuts: text -> kept atoms, without the atom records of the model ----
// process_files reads a file, selects its atoms and throws the model away; building 112-byte atom records with two
// strings each only to walk them once is most of its CPU time.  For PLAIN files - one conformer per residue (no
// alternate-location characters), the records of a chain and of a residue contiguous and in ascending residue order,
// every radius found - the short cuts read the text once and write what prepare() would have written: the kept atoms
// (same order, same f64 -> f32 coordinates, same radii, same ids) and the segment ends, plus a model WITHOUT atoms
// (chains, residues, one named conformer each) for the result's metadata.  Anything else - an alt-loc, a chain or
// residue that comes back, a short record, a missing radius or element, a custom radii table - returns false and the
// file takes the general reader, which also produces the errors.  tests/test_host_api.py compares the two on every
// fixture and on mutated files (`sasa_host_cli prepare`); RSASA_NO_FAST_READER=1 switches it off.
enum class SegKind { None, Residue, Chain };

// What the two short cuts share: the light model and the kept atoms.  A short cut decides by itself (and cheaply) that
// a row belongs to the residue before; it comes here for a new residue and for every atom of the first model.
struct LightModel {
    enum Atom { Kept, Skipped, GiveUp };
    const OptionValues &o;
    const SegKind kind;
    Structure &light;
    Prepared &p;
    const ProtorFlat &protor = protor_flat();
    std::pmr::memory_resource *const mem = light.chains.get_allocator().resource();
    // the current residue, as views of its first row (the model's strings hold the same characters)
    bool have_res = false;
    std::int64_t seq = 0;
    TextView chain{"", 0}, icode{"", 0}, name{"", 0};

    LightModel(const OptionValues &o_, SegKind kind_, Structure &light_, Prepared &p_, size_t expect_atoms)
        : o(o_), kind(kind_), light(light_), p(p_)
    {
        p.atoms.clear();
        p.seg_end.clear();
        p.atoms.reserve(expect_atoms);
    }

    // a new residue: it must continue the current chain in ascending order, or open a chain not seen before
    bool open_residue(const TextView &chain_id, std::int64_t new_seq, const TextView &new_icode, const TextView &res_name)
    {
        if (have_res && same(chain, chain_id)) {
            const int c = std::string_view(icode.first, icode.second).compare(std::string_view(new_icode.first, new_icode.second));
            if (!(new_seq > seq || (new_seq == seq && c < 0))) return false;
        } else {
            for (const Chain &ch : light.chains)
                if (same(ch.id, chain_id)) return false;
            if (kind == SegKind::Chain && have_res) p.seg_end.push_back((uint32_t)p.atoms.size());
            light.chains.push_back(Chain{std::string(chain_id.first, chain_id.second), std::pmr::vector<Residue>(mem)});
        }
        if (kind == SegKind::Residue && have_res) p.seg_end.push_back((uint32_t)p.atoms.size());
        Chain &ch = light.chains.back();
        ch.residues.push_back(Residue{new_seq, std::string(new_icode.first, new_icode.second), std::pmr::vector<Conformer>(mem)});
        ch.residues.back().conformers.push_back(
            Conformer{std::string(res_name.first, res_name.second), std::string(), std::pmr::vector<AtomRecord>(mem)});
        have_res = true;
        seq = new_seq;
        chain = chain_id; icode = new_icode; name = res_name;
        return true;
    }

    // An atom of the current residue.  The element is the symbol in upper case, else the first letter of the name
    // (set_element); it is hydrogen only when it is the one character H, and the van-der-Waals look-up takes the whole
    // symbol.  (A PDB symbol, columns 77-78, has at most two characters: there "one character" is "no second one".)
    // occupancy(), coordinate(0..2) and serial() convert the row's fields when asked: a filtered atom converts nothing.
    template <typename Occupancy, typename Coordinate, typename Serial>
    __attribute__((always_inline)) Atom keep_atom(const TextView &sym, const TextView &atom_name, bool is_het, Occupancy occupancy,
                                                  Coordinate coordinate, Serial serial)
    {
        char e0 = 0;
        if (sym.second) {
            e0 = (char)std::toupper((unsigned char)sym.first[0]);
        } else {
            for (size_t k = 0; k < atom_name.second && !e0; k++)
                if (std::isalpha((unsigned char)atom_name.first[k])) e0 = (char)std::toupper((unsigned char)atom_name.first[k]);
        }
        if (!e0) return GiveUp;                                                       // options.rs:164 (the general path reports it)
        if (!o.include_hydrogens && e0 == 'H' && sym.second <= 1) return Skipped;     // options.rs:166
        if (is_het && !o.include_hetatms) return Skipped;                             // options.rs:169
        float radius = 0.f;
        if (o.read_radii_from_occupancy) {
            radius = (float)occupancy();                                              // options.rs:83-84
        } else if (!protor.find(name, atom_name, &radius)) {
            if (!o.allow_vdw_fallback) return GiveUp;
            std::string el = sym.second ? std::string(sym.first, sym.second) : std::string(1, e0);
            for (auto &c : el) c = (char)std::toupper((unsigned char)c);
            if (!vdw_radius(el, &radius)) return GiveUp;
        }
        rsasa_atom_t a;
        for (int k = 0; k < 3; k++) a.position[k] = (float)coordinate(k);             // options.rs:106-110: f64 -> f32
        a.radius = radius;
        a.id = fnv_id({"", 0}, serial());
        p.atoms.push_back(a);
        return Kept;
    }

    void close()
    {
        if (kind != SegKind::None && have_res) p.seg_end.push_back((uint32_t)p.atoms.size());
    }
};

bool fast_pdb_prepare(const std::string &text, const OptionValues &o, SegKind kind, Structure &light, Prepared &p)
{
    if (o.radii_config) return false;
    LightModel m(o, kind, light, p, text.size() / 80 + 1);
    bool in_first_model = true, seen_model = false;
    std::size_t counter = 0;
    const char *key = nullptr;  // columns 17-27 of the current residue's records
    const char *cur = text.data(), *const end = text.data() + text.size();
    while (cur < end) {
        const LineView line = next_line(cur, end);
        const bool is_atom = line.n >= 6 && std::memcmp(line.p, "ATOM  ", 6) == 0;
        const bool is_het = !is_atom && line.n >= 6 && std::memcmp(line.p, "HETATM", 6) == 0;
        if (!(is_atom || is_het)) {
            if (line.starts_with("MODEL")) {
                if (seen_model) in_first_model = false;
                seen_model = true;
            } else if (line.starts_with("ENDMDL")) {
                in_first_model = false;
            }
            continue;
        }
        if (!in_first_model) continue;
        if (line.n < 54 || line.p[16] != ' ') return false;  // short record / alternate location: the general reader
        counter++;
        if (!key || std::memcmp(line.p + 16, key, 11) != 0) {
            if (!m.open_residue(field_view(line, 22, 22), column_int(line, 23, 26, nullptr), field_view(line, 27, 27), field_view(line, 18, 20)))
                return false;
            key = line.p + 16;
        }
        const LightModel::Atom kept = m.keep_atom(
            field_view(line, 77, 78), field_view(line, 13, 16), is_het, [&] { return column_decimal(line, 55, 60, 1.0, 2); },
            [&](int k) { return column_decimal(line, 31 + 8 * (size_t)k, 38 + 8 * (size_t)k, 0.0, 3); },
            [&] {
                bool ok = false;
                const long v = column_int(line, 7, 11, &ok);
                return ok ? (std::size_t)v : counter;
            });
        if (kept == LightModel::GiveUp) return false;
    }
    m.close();
    return true;
}

// The same short cut for mmCIF text (AlphaFold's files: one `_atom_site` loop, a row per line, no alternate locations):
// the rows' tokens are looked at in place.  The exits are the PDB short cut's: an alternate location, a chain or
// residue that comes back or goes down, a second name inside a residue, a row that is not exactly the header's
// columns, a missing element or radius, a second `_atom_site` loop - the general reader takes the file.

// white space as tokenize_views sees it, one table look-up per character
struct SpaceTable {
    bool is[256] = {};
    SpaceTable() { is[(unsigned char)' '] = true; for (int c = '\t'; c <= '\r'; c++) is[c] = true; }
};
const SpaceTable kSpaceTable;

// tokenize_views into a fixed array (no allocation, no bounds growth); returns the number of tokens, cap + 1 if there
// are more than cap
inline size_t tokenize_row(const char *p, size_t n, TextView *out, size_t cap)
{
    const bool *const sp = kSpaceTable.is;
    size_t i = 0, k = 0;
    while (i < n) {
        while (i < n && sp[(unsigned char)p[i]]) i++;
        if (i >= n) break;
        if (k == cap) return cap + 1;
        if (p[i] == '\'' || p[i] == '"') {
            const char q = p[i++];
            size_t j = i;
            while (j < n && !(p[j] == q && (j + 1 == n || sp[(unsigned char)p[j + 1]]))) j++;
            out[k++] = {p + i, j - i};
            i = j + 1;
        } else {
            size_t j = i + 1;
            while (j < n && !sp[(unsigned char)p[j]]) j++;
            out[k++] = {p + i, j - i};
            i = j;
        }
    }
    return k;
}

// The rows of an `_atom_site` loop are written in aligned columns by most writers (AlphaFold's among them): nearly every
// row has its separators where the row before had them.  RowSplitter keeps the last row's separator mask and token
// bounds; a row with the same mask gets its tokens by adding offsets.  The mask is built sixteen bytes at a time (SSE2);
// rows that hold a quote, a tab or another control character, a byte above 127, or more than 256 bytes - and builds
// without SSE2 - go through tokenize_row.  Either way the tokens are tokenize_views'.
struct RowSplitter {
    static constexpr size_t kMaxCols = 64;
    const char *row = nullptr;          // the current row; token k is row + off[k], len[k] bytes
    uint16_t off[kMaxCols], len[kMaxCols];
    size_t n_tok = 0;
#ifdef RSASA_ROW_SSE2
    uint64_t last_mask[4] = {~0ull, ~0ull, ~0ull, ~0ull};  // bit i: byte i is a blank (or beyond the row's end)
    bool have_last = false;
#endif
    TextView token(size_t k) const { return {row + off[k], len[k]}; }

    // false: more than kMaxCols tokens (or a row too long for 16-bit offsets)
    bool split(const char *p, size_t n, const char *text_end)
    {
        row = p;
#ifdef RSASA_ROW_SSE2
        if (n <= 256) {
            uint64_t m[4] = {~0ull, ~0ull, ~0ull, ~0ull};
            const __m128i blank = _mm_set1_epi8(' '), q1 = _mm_set1_epi8('\''), q2 = _mm_set1_epi8('"');
            unsigned odd = 0;  // quotes, control characters, bytes above 127 (signed compare: below ' ')
            for (size_t b = 0; b < n; b += 16) {
                __m128i v;
                if (p + b + 16 <= text_end) {
                    v = _mm_loadu_si128(reinterpret_cast<const __m128i *>(p + b));
                } else {
                    char tmp[16] = {' ', ' ', ' ', ' ', ' ', ' ', ' ', ' ', ' ', ' ', ' ', ' ', ' ', ' ', ' ', ' '};
                    std::memcpy(tmp, p + b, (size_t)(text_end - (p + b)));
                    v = _mm_loadu_si128(reinterpret_cast<const __m128i *>(tmp));
                }
                uint32_t sp = (uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(v, blank));
                uint32_t bad = (uint32_t)_mm_movemask_epi8(_mm_or_si128(_mm_cmplt_epi8(v, blank), _mm_or_si128(_mm_cmpeq_epi8(v, q1), _mm_cmpeq_epi8(v, q2))));
                if (n - b < 16) {  // bytes beyond the row: blanks, whatever they are
                    const uint32_t in_row = (1u << (n - b)) - 1u;
                    sp |= ~in_row & 0xFFFFu;
                    bad &= in_row;
                }
                odd |= bad;
                m[b >> 6] = (m[b >> 6] & ~(0xFFFFull << (b & 63))) | ((uint64_t)sp << (b & 63));
            }
            if (!odd) {
                if (have_last && m[0] == last_mask[0] && m[1] == last_mask[1] && m[2] == last_mask[2] && m[3] == last_mask[3])
                    return true;  // the previous row's columns: off / len stand
                // token bounds from the mask: every change of state, in order
                size_t k = 0;
                bool in_tok = false;
                size_t start = 0;
                uint64_t carry = 1;  // (the byte before the row counts as a blank)
                for (size_t w = 0; w * 64 < n; w++) {
                    const uint64_t sp = m[w];
                    uint64_t edges = sp ^ ((sp << 1) | carry);
                    carry = sp >> 63;
                    while (edges) {
                        const size_t pos = w * 64 + (size_t)__builtin_ctzll(edges);
                        edges &= edges - 1;
                        if (!in_tok) {
                            if (k == kMaxCols) return false;
                            start = pos;
                        } else {
                            off[k] = (uint16_t)start; len[k] = (uint16_t)(pos - start);
                            k++;
                        }
                        in_tok = !in_tok;
                    }
                }
                if (in_tok) {  // (n is a multiple of 64 and the last token ends with the row)
                    off[k] = (uint16_t)start; len[k] = (uint16_t)(n - start);
                    k++;
                }
                n_tok = k;
                for (int w = 0; w < 4; w++) last_mask[w] = m[w];
                have_last = true;
                return true;
            }
            have_last = false;
        }
#endif
        (void)text_end;
#ifdef RSASA_ROW_SSE2
        have_last = false;  // (off / len are overwritten below: the remembered mask no longer describes them)
#endif
        if (n > 0xFFFFu) return false;
        TextView tmp[kMaxCols];
        n_tok = tokenize_row(p, n, tmp, kMaxCols);
        if (n_tok > kMaxCols) return false;
        for (size_t k = 0; k < n_tok; k++) { off[k] = (uint16_t)(tmp[k].first - p); len[k] = (uint16_t)tmp[k].second; }
        return true;
    }
};

bool fast_cif_prepare(const std::string &text, const OptionValues &o, SegKind kind, Structure &light, Prepared &p)
{
    if (o.radii_config) return false;
    LightModel m(o, kind, light, p, text.size() / 88 + 1);
    AtomSiteHeader h;
    RowSplitter rows;
    auto val = [&](int c) { return c < 0 ? TextView{"", 0} : AtomSiteHeader::value(rows.token((size_t)c)); };
    auto num = [&](int c, double missing) {
        const TextView v = val(c);
        return v.second ? parse_decimal(v.first, v.second) : missing;
    };
    bool had_rows = false;
    std::string first_model;
    const char *cur = text.data(), *const end = text.data() + text.size();
    while (cur < end) {
        const LineView raw = next_line(cur, end);
        const TextView tv = field_view(raw, 1, raw.n);  // trimmed
        if (tv.second == 0) continue;
        const LineView t{tv.first, tv.second};
        const AtomSiteHeader::Line what = h.feed(t);
        if (what == AtomSiteHeader::Column && had_rows) return false;  // a second loop of atoms
        if (what != AtomSiteHeader::Row) continue;
        if (!h.resolved && (!h.resolve() || h.cols.size() > RowSplitter::kMaxCols)) return false;  // (the general reader reports it)
        if (!rows.split(t.p, t.n, end) || rows.n_tok != h.cols.size()) return false;
        had_rows = true;
        const TextView model_id = val(h.model);
        if (first_model.empty()) first_model = model_id.second ? std::string(model_id.first, model_id.second) : "1";
        if (model_id.second && !same(first_model, model_id)) continue;
        if (val(h.alt).second) return false;
        TextView chain_id = val(h.aasym);
        if (!chain_id.second) chain_id = val(h.lasym);
        TextView seq_t = val(h.aseq);
        if (!seq_t.second) seq_t = val(h.lseq);
        const std::int64_t seq = token_long(seq_t);
        const TextView icode = val(h.ins), comp = val(h.comp), group = val(h.group);
        if (m.have_res && same(m.chain, chain_id) && seq == m.seq && same(m.icode, icode)) {
            if (!same(m.name, comp)) return false;  // a second conformer
        } else if (!m.open_residue(chain_id, seq, icode, comp)) {
            return false;
        }
        const bool is_het = group.second == 6 && std::memcmp(group.first, "HETATM", 6) == 0;
        const LightModel::Atom kept = m.keep_atom(
            val(h.sym), val(h.atom), is_het, [&] { return num(h.occ, 1.0); }, [&](int k) { return num(k == 0 ? h.x : k == 1 ? h.y : h.z, 0.0); },
            [&] { return (std::size_t)token_long(val(h.id)); });
        if (kept == LightModel::GiveUp) return false;
    }
    m.close();
    return true;
}

}  // namespace

bool prepare_text(const std::string &text, bool is_cif, const OptionValues &o, int level, bool try_fast,
                  bool skip_occupancy_and_bfactor, Structure &model, Prepared &prep)
{
    static const SegKind kinds[] = {SegKind::None, SegKind::Residue, SegKind::Chain, SegKind::Residue};
    if (try_fast) {  // plain files: kept atoms straight from the text
        Structure light(text.size() / 8 + 4096);
        if (is_cif ? fast_cif_prepare(text, o, kinds[level], light, prep) : fast_pdb_prepare(text, o, kinds[level], light, prep)) {
            model = std::move(light);
            return true;
        }
    }
    model = is_cif ? read_mmcif_text(text, skip_occupancy_and_bfactor) : read_pdb_text(text, skip_occupancy_and_bfactor);
    prep = prepare(model, o, level);
    return false;
}

// Measurement hook (sasa_host_cli prepare-bench-*): seconds per pass of directory mode's per-file work - text to kept
// atoms - through the short cut or the general reader, the file read once; no GPU.
double debug_prepare_seconds(const std::string &path, const OptionValues &o, int level, bool fast, int reps, size_t *n_atoms, bool *used_fast)
{
    const std::string text = read_whole_file(path);
    const bool cif = is_mmcif_path(path);
    size_t atoms = 0;
    bool took_fast = false;
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; r++) {
        Structure model;
        Prepared p;
        took_fast = prepare_text(text, cif, o, level, fast, !o.read_radii_from_occupancy, model, p);
        atoms = p.atoms.size();
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (reps > 0 ? reps : 1);
    if (n_atoms) *n_atoms = atoms;
    if (used_fast) *used_fast = took_fast;
    return s;
}

// Test hook (sasa_host_cli prepare): what directory mode hands to the GPU for one file - kept atoms, segment ends - and
// the model its results take their metadata from, through the short cut (`fast`, when the file qualifies) or the
// general reader (with full records).  JSON text; no GPU.
std::string debug_prepare_json(const std::string &path, const OptionValues &o, int level, bool fast)
{
    Structure model;
    Prepared p;
    const bool used_fast = prepare_text(read_whole_file(path), is_mmcif_path(path), o, level, fast, false, model, p);
    char buf[160];
    std::string out = std::string("{\"fast\":") + (used_fast ? "true" : "false") + ",\"error\":" + std::to_string((int)p.err.error) + ",\"atoms\":[";
    for (size_t i = 0; i < p.atoms.size(); i++) {
        const rsasa_atom_t &a = p.atoms[i];
        std::snprintf(buf, sizeof buf, "%s[\"%a\",\"%a\",\"%a\",\"%a\",\"%llu\"]", i ? "," : "", a.position[0], a.position[1], a.position[2],
                      a.radius, (unsigned long long)a.id);
        out += buf;
    }
    out += "],\"seg_end\":[";
    for (size_t i = 0; i < p.seg_end.size(); i++) out += (i ? "," : "") + std::to_string(p.seg_end[i]);
    out += "],\"model\":[";
    for (size_t c = 0; c < model.chains.size(); c++) {
        out += (c ? ",[\"" : "[\"") + model.chains[c].id + "\",[";
        for (size_t r = 0; r < model.chains[c].residues.size(); r++) {
            const Residue &res = model.chains[c].residues[r];
            std::string name;
            const bool named = res.name(&name);
            out += (r ? ",[" : "[") + std::to_string(res.serial_number) + ",\"" + res.insertion_code + "\",\"" + (named ? name : std::string("?")) + "\"]";
        }
        out += "]]";
    }
    out += "]}";
    return out;
}

// (public, see the header) the ChainLevel selection of one structure without any GPU work
Result<SelectedAtoms> select_by_chain(const Structure &pdb, const OptionValues &o)
{
    Result<SelectedAtoms> r;
    Prepared p = prepare(pdb, o, level_index<ChainLevel>::value);
    if (p.err.error != SASACalcError::Ok) {
        r.error = p.err.error;
        r.message = p.err.message;
        return r;
    }
    r.value.atoms = std::move(p.atoms);
    r.value.chain_end = std::move(p.seg_end);
    for (const Chain &c : pdb.chains) r.value.chain_ids.push_back(c.id);
    return r;
}

}  // namespace detail

Result<SelectedAtoms> select_atoms_by_chain(const Structure &pdb, const OptionValues &o)
{
    return detail::select_by_chain(pdb, o);
}

}  // namespace rustsasa
