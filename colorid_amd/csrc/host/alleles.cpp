// The allele table of a cgMLST scheme from `search -s -m` rows (`search -s -m --alleles PREFIX`, `alleles -r ROWS -o PREFIX`): what the
// reference's workflows/MLST/process_MLST.py derives from the same rows, one pass, one cell per (accession, locus) that occurs.
//   row          label TAB accession TAB n_kmers TAB 1.00 — the accession holds every k-mer of the record `label`
//   locus        the label up to its first '_';  allele: the text between the first and the second '_' (or the end)
//   loci         those that occur in a row, in byte order;  accessions: in order of their first row
//   PREFIX.raw.tsv       header: TAB, then the loci TAB-joined; per accession its name and one cell per locus: the allele, NA for several or none
//   PREFIX.detailed.tsv  the same with MULTI (several rows for the locus, equal alleles included) / NOT_CALLED (none)
//   PREFIX.report.out    acc; total: called/n_loci, multiple: m
//   PREFIX.clean.tsv, PREFIX.dropped.txt   (--max-missing N only) the raw table without / the names of the accessions with more than N NA cells
#include "colorid_host.hpp"

namespace colorid {

void AlleleTable::add(const char *label, size_t label_len, const std::string &accession) {
    const char *u1 = static_cast<const char *>(memchr(label, '_', label_len));
    if (!u1) {
        if (!bad_) { bad_label_.assign(label, label_len); bad_ = true; }
        return;
    }
    const char *rest = u1 + 1, *end = label + label_len;
    const char *u2 = static_cast<const char *>(memchr(rest, '_', (size_t)(end - rest)));
    const std::string locus(label, u1);
    auto it = acc_index_.find(accession);
    if (it == acc_index_.end()) {
        it = acc_index_.emplace(accession, accessions_.size()).first;
        accessions_.push_back(accession);
        cells_.emplace_back();
    }
    loci_.insert(locus);
    Cell &cell = cells_[it->second][locus];
    if (cell.n++ == 0) cell.allele.assign(rest, u2 ? u2 : end);
}

void AlleleTable::add_rows_file(const std::string &path) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) die("alleles: could not open %s", path.c_str());
    char *line = nullptr;
    size_t cap = 0;
    ssize_t n;
    while ((n = getline(&line, &cap, f)) >= 0) {
        size_t len = (size_t)n;
        if (len && line[len - 1] == '\n') --len;
        const char *t1 = static_cast<const char *>(memchr(line, '\t', len));
        if (!t1) continue;
        const char *acc = t1 + 1, *end = line + len;
        const char *t2 = static_cast<const char *>(memchr(acc, '\t', (size_t)(end - acc)));
        if (!t2) continue;
        if (!memchr(t2 + 1, '\t', (size_t)(end - t2 - 1))) continue;   // fewer than four fields: the banner, a warning, an empty line
        add(line, (size_t)(t1 - line), std::string(acc, t2));
    }
    free(line);
    fclose(f);
}

namespace {
FILE *table_out(const std::string &path) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die("alleles: could not create %s", path.c_str());
    setvbuf(f, nullptr, _IOFBF, 1u << 20);
    return f;
}
void table_close(FILE *f, const std::string &path) {
    if (fclose(f) != 0) die("alleles: writing %s failed", path.c_str());
}
}  // namespace

void AlleleTable::write(const std::string &prefix, long long max_missing) const {
    if (bad_)
        die("alleles: the label '%s' has no '_': a scheme's records are named LOCUS_ALLELE; no table is written", bad_label_.c_str());
    const std::vector<std::string> loci(loci_.begin(), loci_.end());   // std::string orders by unsigned bytes
    const std::string raw_path = prefix + ".raw.tsv", det_path = prefix + ".detailed.tsv", rep_path = prefix + ".report.out";
    FILE *raw = table_out(raw_path), *det = table_out(det_path), *rep = table_out(rep_path);
    FILE *clean = nullptr, *dropped = nullptr;
    if (max_missing >= 0) { clean = table_out(prefix + ".clean.tsv"); dropped = table_out(prefix + ".dropped.txt"); }
    std::string header;
    for (const std::string &l : loci) { header += '\t'; header += l; }
    if (loci.empty()) header += '\t';   // ('\t' + '\t'.join([]))
    header += '\n';
    fputs(header.c_str(), raw);
    fputs(header.c_str(), det);
    if (clean) fputs(header.c_str(), clean);
    std::string row, drow;
    for (size_t a = 0; a < accessions_.size(); ++a) {
        const auto &cells = cells_[a];
        size_t multiple = 0, na = 0;
        row = accessions_[a];
        drow = accessions_[a];
        auto it = cells.begin();   // ordered as the loci are: a merge walk
        for (const std::string &l : loci) {
            row += '\t';
            drow += '\t';
            if (it != cells.end() && it->first == l) {
                if (it->second.n == 1) { row += it->second.allele; drow += it->second.allele; }
                else { row += "NA"; drow += "MULTI"; ++multiple; ++na; }
                ++it;
            } else { row += "NA"; drow += "NOT_CALLED"; ++na; }
        }
        row += '\n';
        drow += '\n';
        fputs(row.c_str(), raw);
        fputs(drow.c_str(), det);
        fprintf(rep, "%s; total: %zu/%zu, multiple: %zu\n", accessions_[a].c_str(), cells.size(), loci.size(), multiple);
        if (clean) {
            if ((long long)na > max_missing) fprintf(dropped, "%s\n", accessions_[a].c_str());
            else fputs(row.c_str(), clean);
        }
    }
    table_close(raw, raw_path);
    table_close(det, det_path);
    table_close(rep, rep_path);
    if (clean) { table_close(clean, prefix + ".clean.tsv"); table_close(dropped, prefix + ".dropped.txt"); }
    fprintf(stderr, "alleles: %zu accessions x %zu loci written to %s, %s and %s\n", accessions_.size(), loci.size(), raw_path.c_str(),
            det_path.c_str(), rep_path.c_str());
}

// ---------------------------------------------------------------- PREFIX.nearest.tsv (`search -s -m --alleles PREFIX --nearest`)

void NearestTable::add_record(const std::string &label) {
    if (!bad_ && label.find('_') == std::string::npos) { bad_label_ = label; bad_ = true; }
    labels_.push_back(label);
}

// `later` holds records after the cell's: it wins only with a strictly greater share, hits_a * len_b against hits_b * len_a in 64 bits
void NearestTable::merge(cid_nearest &cell, const cid_nearest &later) {
    const uint32_t n_perfect = cell.n_perfect + later.n_perfect;
    if (later.seg != CID_NEAREST_NONE &&
        (cell.seg == CID_NEAREST_NONE || (uint64_t)later.kmers_hit * cell.n_kmers > (uint64_t)cell.kmers_hit * later.n_kmers))
        cell = later;
    cell.n_perfect = n_perfect;
}

void NearestTable::merge_group(const std::string &locus, const cid_nearest *cells, size_t record_base) {
    auto it = loci_.find(locus);
    if (it == loci_.end()) it = loci_.emplace(locus, std::vector<cid_nearest>(n_colors_, cid_nearest{CID_NEAREST_NONE, 0, 0, 0})).first;
    for (size_t c = 0; c < n_colors_; ++c) {
        cid_nearest in = cells[c];
        if (in.seg != CID_NEAREST_NONE) in.seg += (uint32_t)record_base;
        merge(it->second[c], in);
    }
}

void NearestTable::write(const std::string &prefix, const std::vector<std::string> &accessions, double min_share) const {
    if (bad_)
        die("alleles: the label '%s' has no '_': a scheme's records are named LOCUS_ALLELE; no nearest-allele file is written", bad_label_.c_str());
    const std::string path = prefix + ".nearest.tsv";
    FILE *f = table_out(path);
    fputs("accession\tlocus\tallele\tkmers_hit\tkmers\tshare\n", f);
    size_t n = 0;
    for (size_t c = 0; c < n_colors_; ++c)
        for (const auto &lc : loci_) {   // std::string orders by unsigned bytes
            const cid_nearest &cell = lc.second[c];
            if (cell.n_perfect || cell.seg == CID_NEAREST_NONE) continue;
            const double share = (double)cell.kmers_hit / (double)cell.n_kmers;
            if (!(share >= min_share)) continue;
            const std::string &label = labels_[cell.seg];
            const size_t u1 = label.find('_'), u2 = label.find('_', u1 + 1);
            fprintf(f, "%s\t%s\t%s\t%u\t%u\t%.3f\n", accessions[c].c_str(), lc.first.c_str(),
                    label.substr(u1 + 1, u2 == std::string::npos ? std::string::npos : u2 - u1 - 1).c_str(), cell.kmers_hit, cell.n_kmers, share);
            ++n;
        }
    table_close(f, path);
    fprintf(stderr, "alleles: %zu nearest-allele calls (share >= %g) written to %s\n", n, min_share, path.c_str());
}

}  // namespace colorid
