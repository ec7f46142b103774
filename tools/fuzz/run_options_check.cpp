// run_options_check.cpp — csvhost_run_options (contextsv_amd/csrc/host/abi/csvhost_abi.h) against RunParams (sv_caller.h), on the CPU under
// AddressSanitizer + UBSan (make options-check): csvhost_run_options_init followed by run_params_from gives a default-constructed RunParams;
// every field of the struct, changed alone, changes the RunParams / RunSchedule field of its own name and no other; a wrong size and an
// early_batches outside 0-3 are refused. Links host/abi/options.cpp only: the decoder is inline and touches nothing but fields.
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../contextsv_amd/csrc/host/abi/csvhost_abi.h"
#include "../../contextsv_amd/csrc/host/abi/run_options.hpp"
#include "../../contextsv_amd/csrc/host/sv_caller.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Field { std::string option, member; bool is_bool, is_real; };

static std::vector<Field> fields()
{
    std::vector<Field> f;
#define X(field, member, type) f.push_back({#field, #member, std::is_same<type, bool>::value, std::is_floating_point<type>::value});
    CSVHOST_RUN_OPTION_FIELDS(X)
#undef X
    return f;
}
// every mapped field of P, in the table's order
static std::vector<double> mapped(const RunParams &P)
{
    std::vector<double> v;
#define X(field, member, type) v.push_back((double)P.member);
    CSVHOST_RUN_OPTION_FIELDS(X)
#undef X
    return v;
}
// what the run options do not reach stays as RunParams makes it
static bool rest_is_default(const RunParams &P)
{
    const RunParams D;
    return P.cigar_svs == D.cigar_svs && P.snp_vcf.empty() && P.pfb_table.empty() && P.ethnicity.empty() && !P.ref_genome && P.vcf.output_dir.empty() &&
           P.vcf.assembly_gaps.empty() && P.vcf.file_date.empty();
}
// field `at` of o set to `value`
static void set_field(csvhost_run_options &o, size_t at, double value)
{
    size_t k = 0;
#define X(field, member, type) if (k++ == at) o.field = (decltype(o.field))value;
    CSVHOST_RUN_OPTION_FIELDS(X)
#undef X
}
static bool refused(const csvhost_run_options &o)
{
    try { run_params_from(o); } catch (const std::invalid_argument &) { return true; }
    return false;
}

int main()
{
    const std::vector<Field> F = fields();
    // the table names every field behind `size`: two doubles, the rest 32-bit, and `size` padded to the doubles' alignment
    CHECK(sizeof(csvhost_run_options) == 8 + 2 * 8 + 4 * (F.size() - 2), "the struct has fields the table does not name: %zu bytes, %zu fields", sizeof(csvhost_run_options), F.size());
    for (const Field &f : F) {
        const std::string tail = f.member.substr(f.member.rfind('.') == std::string::npos ? 0 : f.member.rfind('.') + 1);
        CHECK(tail == f.option, "%s is mapped to %s", f.option.c_str(), f.member.c_str());
    }

    csvhost_run_options o;
    memset(&o, 0xff, sizeof o);
    csvhost_run_options_init(&o);
    CHECK(o.size == sizeof o, "init wrote size %u", o.size);
    const RunParams P0 = run_params_from(o);
    const std::vector<double> d = mapped(RunParams()), m0 = mapped(P0);
    for (size_t i = 0; i < F.size(); i++) CHECK(m0[i] == d[i], "init + decode: %s = %g, RunParams has %g", F[i].option.c_str(), m0[i], d[i]);
    CHECK(rest_is_default(P0), "init + decode touched a field that is no run option");

    for (size_t i = 0; i < F.size(); i++) {
        const double changed = F[i].is_bool ? 1.0 - d[i] : F[i].is_real ? d[i] + 0.25 : F[i].option == "early_batches" ? 3.0 : d[i] + 3.0;
        csvhost_run_options o1 = o;
        set_field(o1, i, changed);
        const RunParams P1 = run_params_from(o1);
        const std::vector<double> m1 = mapped(P1);
        for (size_t k = 0; k < F.size(); k++)
            CHECK(m1[k] == (k == i ? changed : d[k]), "%s = %g: %s is %g", F[i].option.c_str(), changed, F[k].member.c_str(), m1[k]);
        CHECK(rest_is_default(P1), "%s touched a field that is no run option", F[i].option.c_str());
    }
    // a flag is anything but 0
    { csvhost_run_options o1 = o; o1.save_cnv = 2; CHECK(run_params_from(o1).save_cnv, "save_cnv = 2 reads as off"); }

    for (int eb = 0; eb <= 3; eb++) { csvhost_run_options o1 = o; o1.early_batches = eb; CHECK(!refused(o1) && (int)run_params_from(o1).schedule.early_batches == eb, "early_batches %d", eb); }
    for (int eb : {-1, 4, 1 << 20}) { csvhost_run_options o1 = o; o1.early_batches = eb; CHECK(refused(o1), "early_batches %d was taken", eb); }
    for (uint32_t size : {0u, (uint32_t)sizeof o - 4, (uint32_t)sizeof o + 4}) { csvhost_run_options o1 = o; o1.size = size; CHECK(refused(o1), "size %u was taken", size); }

    printf("run_options_check: %zu fields, %d failures\n", F.size(), failures);
    return failures ? 1 : 0;
}
