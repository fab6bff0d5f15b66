/*
 * pseudoaligner_amd.h — C ABI of the MI355X-native pseudoalignment hot path.
 *
 * This is the drop-in boundary for ONE path of 10XGenomics/rust-pseudoaligner
 * (crate `debruijn_mapping` v0.6.0): per-read k-mer lookup + De Bruijn graph
 * extension + equivalence-class intersection, i.e.
 *
 *     Pseudoaligner::map_read                 src/pseudoaligner.rs:381-384
 *       -> map_read_with_mismatch             src/pseudoaligner.rs:361-376
 *          -> map_read_to_nodes_with_mismatch src/pseudoaligner.rs:64-319
 *          -> nodes_to_eq_class / intersect   src/pseudoaligner.rs:323-356, 389-418
 *     process_reads (driver)                  src/pseudoaligner.rs:420-514
 *
 * The reference has no FFI of its own (it is a pure-Rust crate); the symbols
 * below are what a Rust `extern "C"` block would bind to replace the body of
 * `process_reads` / `map_read` (see INTEGRATION.md for the binding).
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types; every function returns
 *     0 (PA_OK) or a negative pa_status; the message of the last failure on the
 *     calling thread is available from pa_last_error().
 *   - nothing aborts or throws across the ABI (the reference panics instead:
 *     src/pseudoaligner.rs:307,446,464).
 *   - bases are 2-bit codes A=0 C=1 G=2 T=3, packed LSB-first: base j of a
 *     sequence lives in bits [2*(j%32), 2*(j%32)+1] of 64-bit word j/32.
 *   - "device" pointers are HIP device pointers on the GPU the index lives on;
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream).
 */
#ifndef PSEUDOALIGNER_AMD_H
#define PSEUDOALIGNER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_ABI_VERSION 1u

/* config.rs:16-18 — the three constants that parameterise the hot path. */
#define PA_READ_COVERAGE_THRESHOLD 32u   /* src/config.rs:16 */
#define PA_LEFT_EXTEND_NUM 1u            /* LEFT_EXTEND_FRACTION = 0.2 = 1/5, src/config.rs:17 */
#define PA_LEFT_EXTEND_DEN 5u
#define PA_DEFAULT_ALLOWED_MISMATCHES 2u /* src/config.rs:18 */
#define PA_SEEK_STRIDE 3u                /* `*kmer_pos += 3`, src/pseudoaligner.rs:110 */

#define PA_NO_EDGE 0xFFFFFFFFu
#define PA_MIN_K 8u
#define PA_MAX_K 64u                     /* one or two 64-bit words per k-mer (Kmer20..Kmer32, Kmer48, Kmer64 of the debruijn crate) */
#define PA_MAX_READ_LEN 1048575u         /* 2^20 - 1 bases. The reference has no limit: its validate_dbg maps whole transcripts (src/build_index.rs:309; the
                                            longest of GENCODE are a few hundred kb). Reads of more than 512 bases stay in their HBM tile while they are
                                            mapped and take the wide lane state (28-bit positions: csrc/lane_steps.hpp); per slot of the pool such a launch
                                            keeps 8 x length words of class-list scratch, so the grid shrinks with the length (a batch of Mb reads is
                                            mapped by a handful of waves: completeness, not throughput) */
#define PA_MAX_SIM_READ_LEN 2048u        /* pa_simulate_reads_*: longest synthetic read */

typedef enum pa_status {
    PA_OK = 0,
    PA_ERR_INVALID_ARG = -1,
    PA_ERR_IO = -2,
    PA_ERR_FORMAT = -3,        /* malformed FASTA/FASTQ or inconsistent flat index */
    PA_ERR_NO_DEVICE = -4,     /* HIP runtime / GPU not usable: the product never falls back to a CPU path */
    PA_ERR_HIP = -5,
    PA_ERR_OOM = -6,
    PA_ERR_ARENA_FULL = -7,    /* caller-provided class arena too small; required size reported */
    PA_ERR_UNSUPPORTED = -8,
    PA_ERR_INTERNAL = -9,
    PA_ERR_BUFFER_TOO_SMALL = -10,  /* pa_records_pull: the caller's buffer cannot hold even the next tuple; *n_bytes = the bytes it needs */
    PA_ERR_NOT_BGZF = -11           /* pa_bgzf_scan: the bytes are not BGZF from first to last (ordinary gzip, a truncated member, ...) */
} pa_status;

/* ------------------------------------------------------------------------------------------
 * Flat index: the interchange form of `pub struct Pseudoaligner<K>` (src/pseudoaligner.rs:26-33).
 * A Rust exporter fills it from the struct's pub fields (dbg, eq_classes); `dbg_index` (the boomphf
 * MPHF, :30) is NOT part of the interchange because every hit is verified against the node sequence
 * (:99-107), which makes it equivalent to an exact k-mer dictionary that the library rebuilds.
 * All arrays are borrowed for the duration of the call that receives the struct.
 * ------------------------------------------------------------------------------------------ */
typedef struct pa_flat_index {
    uint32_t k;                  /* K::k() */
    uint32_t num_nodes;          /* dbg.len() */
    uint32_t num_classes;        /* eq_classes.len() */
    uint32_t num_transcripts;    /* tx_names.len() */
    uint64_t seq_bases;          /* sum of node_len */
    const uint64_t* node_seq;    /* packed bases of all nodes back to back (node i starts at base node_start[i]) */
    const uint64_t* node_start;  /* [num_nodes + 1] base offsets into node_seq */
    const uint32_t* node_len;    /* [num_nodes] node.len() in bases (>= k) */
    const uint8_t*  node_exts;   /* [num_nodes] debruijn::Exts byte: bit b = right ext b, bit 4+b = left ext b */
    const uint32_t* node_colour; /* [num_nodes] *node.data() = equivalence-class id */
    const uint64_t* ec_offset;   /* [num_classes + 1] CSR offsets into ec_ids */
    const uint32_t* ec_ids;      /* eq_classes[c] = ec_ids[ec_offset[c] .. ec_offset[c+1]) sorted, dedup'd */
    /* optional (may be NULL): edges as node.r_edges()/l_edges() would resolve them, indexed by BASE
     * (not by rank): node_redge[4*i + b] = r_edges()[rank of b among set right exts].0, PA_NO_EDGE when
     * the ext bit is clear. When NULL the library derives them the way the debruijn crate does (look up
     * the terminal k-mer extended by b). */
    const uint32_t* node_redge;  /* [4 * num_nodes] */
    const uint32_t* node_ledge;  /* [4 * num_nodes] */
} pa_flat_index;

/* ---------------- host-side index (CPU; "index construction stays on the CPU") ---------------- */
typedef struct pa_host_index pa_host_index;

/* build_index (src/build_index.rs:27-91) + utils::read_transcripts (src/utils.rs:61-97):
 * FASTA -> stranded coloured compacted De Bruijn graph + equivalence classes. */
int pa_host_index_build_fasta(const char* fasta_path, uint32_t k, int num_threads, pa_host_index** out);
/* same from already packed transcripts: tx_start[num_tx+1] base offsets into `packed`. */
int pa_host_index_build_packed(const uint64_t* packed, const uint64_t* tx_start, uint32_t num_tx,
                               uint32_t k, int num_threads, pa_host_index** out);
/* The same two builders with the graph construction on HIP device `device` (k-mer enumeration, radix sort,
 * colour interning, unitig compaction by pointer jumping — csrc/index_build.hip). The result is the SAME index, array for
 * array, as the CPU builders give (src/build_index.rs:27-91 semantics; numbering as in csrc/dbg_build.cpp).
 * PA_ERR_NO_DEVICE without a GPU; PA_ERR_UNSUPPORTED beyond 2^24 transcripts or 2^32 k-mer occurrences. */
int pa_host_index_build_fasta_device(const char* fasta_path, uint32_t k, int device, pa_host_index** out);
int pa_host_index_build_packed_device(const uint64_t* packed, const uint64_t* tx_start, uint32_t num_tx,
                                      uint32_t k, int device, pa_host_index** out);
/* wrap caller arrays (deep copy) — the import path for an index exported from the Rust side. */
int pa_host_index_from_flat(const pa_flat_index* flat, pa_host_index** out);
int pa_host_index_view(const pa_host_index* h, pa_flat_index* view);   /* pointers valid until destroy */
/* The diff tool of the interchange (an index exported from the Rust side vs the one built here from the same FASTA):
 * 0 = equivalent, 1 = different, 2 = undecided (node sets differ and the k-mer level check would exceed max_kmers),
 * < 0 error. Node / class numbering and node order are free; compared are the nodes as a set of (sequence, extension bits,
 * class id LIST) and, when only unitig break points differ, the k-mer -> id-list map. `report` gets one line of text. */
int pa_host_index_compare(const pa_host_index* a, const pa_host_index* b, uint64_t max_kmers, char* report, size_t report_cap);
int pa_host_index_save(const pa_host_index* h, const char* path);      /* own little-endian container, not bincode */
int pa_host_index_load(const char* path, pa_host_index** out);
/* transcript metadata: tx_names (:31) and the gene of each transcript (:32) */
uint32_t pa_host_index_num_transcripts(const pa_host_index* h);
const char* pa_host_index_tx_name(const pa_host_index* h, uint32_t tx);
const char* pa_host_index_tx_gene(const pa_host_index* h, uint32_t tx);
/* Gene-level collapse of the class-count table through tx_gene_mapping (src/pseudoaligner.rs:32; the reference stores the
 * mapping and leaves the collapse to its callers). Genes are numbered by first appearance in transcript order.
 *   pa_host_index_genes            tx_gene[num_transcripts] (may be NULL) and the number of genes
 *   pa_host_index_gene_name        name of gene g
 *   pa_counts_collapse_genes       gene_counts[g] += class_counts[c] for every class c whose transcripts all belong to gene
 *                                  g; classes that span several genes go to gene_counts[num_genes]; the three tail slots
 *                                  of the class table (novel / empty / unmapped, pa_counts_len) are not gene-resolvable
 *                                  and are skipped. gene_counts has num_genes + 1 entries and is NOT cleared. */
int pa_host_index_genes(const pa_host_index* h, uint32_t* tx_gene, uint32_t* num_genes);
const char* pa_host_index_gene_name(const pa_host_index* h, uint32_t gene);
int pa_counts_collapse_genes(const pa_host_index* h, const uint64_t* class_counts, uint64_t counts_len, uint64_t* gene_counts);
/* Mappability of every transcript (analyze_graph, src/mappability.rs:120-156; `pseudoaligner mappability`,
 * src/bin/pseudoaligner.rs:152-172): a node of L bases holds L - K + 1 k-mers shared by the transcripts of its class.
 *   tx_mult[t * PA_MAPPABILITY_COUNTS_LEN + min(j, LEN) - 1]   k-mers of transcript t whose class has j transcripts
 *   gene_mult[t * PA_MAPPABILITY_COUNTS_LEN + min(g, LEN) - 1] k-mers of transcript t whose class spans g distinct genes
 * Both arrays have num_transcripts * PA_MAPPABILITY_COUNTS_LEN entries and are overwritten; either may be NULL.
 * pa_write_mappability_tsv writes the reference's tx_mappability.tsv (write_mappability_tsv, src/mappability.rs:91-104:
 * header + "tx_name gene_name tx_kmer_count frac_kmer_unique_tx frac_kmer_unique_gene", tab separated, fractions printed
 * like Rust's `{}` of an f64: shortest round-trip digits, fixed notation, "NaN" for a transcript without k-mers). */
#define PA_MAPPABILITY_COUNTS_LEN 11   /* src/config.rs:23 */
int pa_host_index_mappability(const pa_host_index* h, uint64_t* tx_mult, uint64_t* gene_mult);
int pa_write_mappability_tsv(const pa_host_index* h, const char* path);
/* packed transcripts the index was built from (kept for read simulation / validation) */
int pa_host_index_transcripts(const pa_host_index* h, const uint64_t** packed, const uint64_t** tx_start,
                              uint32_t* num_tx);
void pa_host_index_destroy(pa_host_index* h);

/* ---------------- device index ---------------- */
typedef struct pa_index pa_index;

typedef struct pa_index_stats {
    uint64_t num_kmers;        /* distinct k-mers = dictionary entries */
    uint64_t table_slots;      /* dictionary capacity (16-byte slots) */
    uint64_t bytes_table, bytes_graph, bytes_classes, bytes_total;
    uint32_t num_nodes, num_classes, k, max_class_len;
} pa_index_stats;

/* Flatten for the GPU and upload to HIP device `device`. Fails with PA_ERR_NO_DEVICE when no GPU. */
int pa_index_create(const pa_flat_index* flat, int device, pa_index** out);
/* The same for several GPUs of one process (`devices, ndev`): out[i] receives the handle of devices[i]; the
 * index is replicated (reads shard over the handles, §8e). All or nothing: on failure every handle created so far is
 * destroyed and out[] is NULL throughout. A host that runs one process per GPU calls pa_index_create instead. */
int pa_index_create_multi(const pa_flat_index* flat, const int* devices, int ndev, pa_index** out);
int pa_index_get_stats(const pa_index* idx, pa_index_stats* stats);
void pa_index_destroy(pa_index* idx);

/* ---------------- read batches ---------------- */
/* Device tile layout ("coalesced HBM tiles"): reads are grouped 64 to a tile; a tile holds
 * `words_per_read` 64-bit words per read, word-major: tiles[(t*words_per_read + w)*64 + r] is word w of
 * read 64*t + r. lens[i] is the length in bases of read i. n_reads need not be a multiple of 64 but the
 * tile buffer must be sized for ceil(n/64) whole tiles. */
typedef struct pa_read_result {   /* one per read, same order as the input */
    uint32_t coverage;            /* map_read .1 (bases aligned); 0 when unmapped */
    uint32_t mismatches;          /* map_read_with_mismatch .2; bit 31 = mapped (Some vs None) */
    uint32_t class_off;           /* where the class (map_read .0) is: bit 31 set = it IS index class (class_off & 0x7FFFFFFF),
                                     i.e. eq_classes[id] of the flat index, returned by reference; bit 31 clear = offset of
                                     the ids in the arena (u32 units): an intersection that is no single visited class */
    uint32_t class_len;           /* number of transcript ids */
} pa_read_result;
#define PA_MAPPED_BIT 0x80000000u
#define PA_CLASS_REF 0x80000000u
/* Arena offsets must leave bit 31 of class_off free: a launch uses at most this many arena entries, however large the
 * caller's buffer is (a batch that needs more fails with PA_ERR_ARENA_FULL: split it). */
#define PA_MAX_ARENA_ENTRIES 0x7FFFFFFFull

size_t pa_tiles_words(uint64_t n_reads, uint32_t words_per_read);   /* u64 words in the tile buffer */
uint32_t pa_words_per_read(uint32_t max_read_len);

/* DnaString::from_dna_string (src/pseudoaligner.rs:449-450) for a batch, on the GPU:
 * ASCII reads (concatenated, offsets[n+1]) already on the device -> tiles + lens. */
int pa_encode_reads_device(const pa_index* idx, const uint8_t* d_ascii, const uint64_t* d_offsets, uint64_t n_reads,
                           uint32_t words_per_read, uint64_t* d_tiles, uint32_t* d_lens, void* stream);
/* host reference of the same packing (used by the host driver for the single-read path and by tests) */
int pa_encode_reads_host(const uint8_t* ascii, const uint64_t* offsets, uint64_t n_reads, uint32_t words_per_read,
                         uint64_t* tiles, uint32_t* lens);

/* The hot path. map_read_with_mismatch for every read of a device-resident batch.
 *   d_results  [n_reads] pa_read_result
 *   d_arena    [arena_cap] u32: ids of the classes that are not index classes, referenced by (class_off, class_len)
 *   d_colour   optional [n_reads] u32: equivalence-class id of the result when it equals an index class
 *              reached by the read, 0xFFFFFFFF otherwise (input of pa_counts_accumulate_device); may be NULL
 * Asynchronous on `stream`; completion status is fetched with pa_map_finish(idx, stream, ...) (which synchronises that
 * stream). The index is immutable and shareable: launches on DIFFERENT streams — from one host thread or several — run
 * concurrently (every stream gets its own control block, list-mode rows and result streams inside the handle; two launches may
 * accumulate into one d_counts). Launches on ONE stream are ordered by the stream and share a control block: call
 * pa_map_finish between them if you need each launch's own status / arena use. */
int pa_map_batch_device(pa_index* idx, const uint64_t* d_tiles, const uint32_t* d_lens, uint64_t n_reads,
                        uint32_t words_per_read, uint32_t allowed_mismatches, pa_read_result* d_results,
                        uint32_t* d_arena, uint64_t arena_cap, uint32_t* d_colour, void* stream);
/* Same launch with the class-count table fused in: d_counts[pa_counts_len(idx)] (u64, caller-owned so that it can be
 * all-reduced with RCCL) is incremented once per read as pa_counts_accumulate_device would. On PA_ERR_ARENA_FULL every
 * read of that launch is still counted once, but a list-mode result whose ids did not fit cannot be looked up by content
 * and lands in the "novel" slot; the class ids are incomplete. Re-run the batch with the arena pa_map_finish asks for —
 * into a table restored to its value before the failed launch (snapshot it, or count into a scratch table and add it on
 * success): the failed launch has already added its reads. */
int pa_map_count_batch_device(pa_index* idx, const uint64_t* d_tiles, const uint32_t* d_lens, uint64_t n_reads,
                              uint32_t words_per_read, uint32_t allowed_mismatches, pa_read_result* d_results,
                              uint32_t* d_arena, uint64_t arena_cap, uint64_t* d_counts, void* stream);
/* The same launch for a batch whose reads all have `read_len` bases (what a sequencer run delivers): no per-read length array — 4 of
 * the 44 bytes per 150-base read that cross PCIe in the host-to-host pipeline, and one request stream less inside the kernel. */
int pa_map_count_batch_uniform_device(pa_index* idx, const uint64_t* d_tiles, uint32_t read_len, uint64_t n_reads,
                                      uint32_t words_per_read, uint32_t allowed_mismatches, pa_read_result* d_results,
                                      uint32_t* d_arena, uint64_t arena_cap, uint64_t* d_counts, void* stream);
/* Synchronise and report: PA_OK, or PA_ERR_ARENA_FULL with *arena_needed set (re-run with a larger arena).
 * *arena_used = entries of d_arena that may hold ids (never more than the arena_cap of the launch). */
int pa_map_finish(pa_index* idx, void* stream, uint64_t* arena_used, uint64_t* arena_needed);
/* Per-stream scratch: the first launch on a stream creates that stream's launch context inside the handle and keeps it for
 * later launches on the same stream: a control block; list-mode rows of CUs x 3 x 4 waves x 128 slots x (256 x words_per_read
 * + 24) x 4 bytes (about 2 GB at 150 bp on a 256-CU part); the stream of reads whose class is looked up by content after the
 * mapping kernel, sized for the worst case (32 bytes per read of the largest launch); and for class-count launches the key
 * streams (about 13 bytes per read) and, with an overflow table attached, the novel list (8 bytes per read) — some 4.5 GB for
 * 100 M-read launches. pa_index_release_stream frees it (after synchronising the stream): call it before destroying a stream
 * you launched on; pa_index_destroy frees what is left. A host that launches from a pool of N streams holds N contexts. */
int pa_index_release_stream(pa_index* idx, void* stream);
/* Measurement (bench.py's roofline leg): with timing on, every launch records HIP events around its mapping kernel on the launch
 * stream; pa_map_kernel_ms returns the duration of the last launch's mapping kernel on `stream` (it waits for that kernel).
 * The class-count kernels of pa_map_count_batch_device run after the second event. */
int pa_index_set_timing(pa_index* idx, int on);
int pa_map_kernel_ms(pa_index* idx, void* stream, float* ms);
/* The three stages of the last timed launch on `stream`, in ms: ms[0] the mapping kernel, ms[1] the kernel that resolves the
 * deferred content lookups (it writes the records of the reads whose class is looked up by content: part of mapping the
 * batch), ms[2] the class-count kernels (zero-length for launches without a count table). Waits for the launch. */
int pa_map_stage_ms(pa_index* idx, void* stream, float ms[3]);
/* arena capacity (u32 entries) that suffices for typical batches of n_reads; the exact need is data dependent */
uint64_t pa_map_arena_hint(const pa_index* idx, uint64_t n_reads);

/* Compact records for the way back to the host (SURVEY.md §8d measures host to host; the 16-byte records are 40 % of what a 150-base read
 * costs the link in the other direction): what map_read_with_mismatch returns (src/pseudoaligner.rs:361-376) in 8 bytes per read,
 *   bits  0..13  coverage        bits 14..27  mismatches        bit 28  mapped (Some / None)
 *   bit  29      PA_COMPACT_BY_REF: the class IS index class (record >> 32), i.e. eq_classes[id] of the flat index
 *   bit  30      PA_COMPACT_PACKED: the class is no index class: its ids are the next entry of the PACKED stream — entries {length, id0,
 *                id1, ...} back to back in READ order (record >> 32 = the entry's word offset in the packed stream of its launch, modulo 2^32;
 *                a reader that walks the records in order needs none of it)
 *   neither bit: the class is empty (or the read unmapped); both bits: the ids did not fit the launch's arena (pa_map_finish said so)
 * made from a launch's records and arena on the device: d_compact[n_reads] u64, d_packed[packed_cap] u32, *d_packed_words (device u64) =
 * words the packed stream needs (entries that would end beyond packed_cap are not written). d_scratch: pa_compact_scratch_bytes(n_reads)
 * bytes. Asynchronous on `stream`, behind the launch that wrote d_results. It cannot fail per record: direct callers must not feed it
 * results of reads longer than PA_COMPACT_MAX_READ_LEN bases — beyond that length the two 14-bit fields hold the low 14 bits of
 * coverage and mismatches. */
#define PA_COMPACT_MAPPED 0x10000000u
#define PA_COMPACT_BY_REF 0x20000000u
#define PA_COMPACT_PACKED 0x40000000u
#define PA_COMPACT_MAX_READ_LEN 16383u   /* compact records carry coverage and mismatches in 14 bits each: they are exact only for reads of at most this many
                                          * bases. Bounding the length bounds both fields: every unit of coverage and every counted mismatch of
                                          * map_read_to_nodes_with_mismatch (src/pseudoaligner.rs:64-319) belongs to a read base of its own — the left extension
                                          * compares bases in front of the first matching k-mer, the forward search only bases behind it, each once — so neither
                                          * exceeds the read's length, whatever allowed_mismatches is. pa_map_tiles_host refuses longer reads. */
size_t pa_compact_scratch_bytes(uint64_t n_reads);
int pa_results_compact_device(pa_index* idx, const pa_read_result* d_results, const uint32_t* d_arena, uint64_t arena_cap, uint64_t n_reads,
                              uint64_t* d_compact, uint32_t* d_packed, uint64_t packed_cap, uint64_t* d_packed_words, void* d_scratch,
                              size_t scratch_bytes, void* stream);

/* The hot path HOST TO HOST (SURVEY.md §8d's literal metric): a batch that lies in host memory in the tile layout — pinned memory
 * (pa_host_alloc_pinned, hipHostMalloc, hipHostRegister) for the copies to run at the link's rate and beside the kernels — mapped in chunks
 * of chunk_reads reads (0: 1 M) that rotate over n_streams streams of the handle (0: 4; at most 8): the copy of chunk i + 1 to the GPU, the
 * kernels of chunk i and the copy of chunk i - 1's outputs back overlap. h_lens NULL: every read has uniform_len bases (no length array
 * crosses the link). Outputs in read order: h_compact[n_reads] (the 8-byte records above), h_packed[*packed_words] (their packed classes;
 * PA_ERR_ARENA_FULL when packed_cap is too small), h_counts[pa_counts_len(idx)] (the class-count table of the batch, overwritten; may
 * be NULL). Synchronous: everything has arrived when the call returns. Streams and staging buffers stay parked on the handle. A read
 * longer than PA_COMPACT_MAX_READ_LEN bases (uniform_len, or any h_lens[i]) does not fit the compact records: PA_ERR_INVALID_ARG, before
 * anything is copied or launched. */
int pa_map_tiles_host(pa_index* idx, const uint64_t* h_tiles, const uint32_t* h_lens, uint32_t uniform_len, uint64_t n_reads,
                      uint32_t words_per_read, uint32_t allowed_mismatches, uint64_t* h_compact, uint32_t* h_packed, uint64_t packed_cap,
                      uint64_t* packed_words, uint64_t* h_counts, uint64_t chunk_reads, int n_streams);
int pa_host_alloc_pinned(size_t bytes, void** out);
int pa_host_free_pinned(void* p);

/* Host-buffer convenience (H2D, map, D2H; grows its own arena). results[n], class ids returned as a
 * CSR in read order: class_offsets[n+1], class_ids (library-owned, valid until the next call on idx
 * from this thread or pa_index_destroy). Reads are ASCII, concatenated, offsets[n+1]. */
int pa_map_batch(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n_reads,
                 uint32_t allowed_mismatches, pa_read_result* results, uint64_t* class_offsets,
                 const uint32_t** class_ids);
/* The same for reads the caller already holds 2-bit packed — what `DnaString::from_dna_string` made of the record (:450) and
 * what `map_read(&self, read_seq: &DnaString)` (:381) receives: no ASCII round trip. Read i = lens[i] bases in the words
 * words[word_offsets[i] .. word_offsets[i+1]) (every read starts on a word boundary; bases beyond the length are ignored).
 * layout 0: this library's words (base j in bits 2 (j % 32) of word j / 32); layout 1: MSB-first words (base j in bits
 * 62 - 2 (j % 32)), the storage order of the debruijn crate's DnaString as far as it is known here. */
#define PA_PACKED_LSB_FIRST 0
#define PA_PACKED_MSB_FIRST 1
int pa_map_batch_packed(pa_index* idx, const uint64_t* words, const uint64_t* word_offsets, const uint32_t* lens, uint64_t n_reads,
                        int layout, uint32_t allowed_mismatches, pa_read_result* results, uint64_t* class_offsets,
                        const uint32_t** class_ids);
/* map_read_with_mismatch (:361) / map_read (:381) of one packed read: returns 1 = Some, 0 = None, <0 error. */
int pa_map_read_packed(pa_index* idx, const uint64_t* words, uint32_t len, int layout, uint32_t allowed_mismatches,
                       uint32_t* class_buf, uint32_t class_cap, uint32_t* class_len, uint32_t* coverage, uint32_t* mismatches);
/* map_read (src/pseudoaligner.rs:381): returns 1 = Some, 0 = None, <0 error. */
int pa_map_read(pa_index* idx, const uint8_t* ascii, uint32_t len, uint32_t* class_buf, uint32_t class_cap,
                uint32_t* class_len, uint32_t* coverage);
int pa_map_read_with_mismatch(pa_index* idx, const uint8_t* ascii, uint32_t len, uint32_t allowed_mismatches,
                              uint32_t* class_buf, uint32_t class_cap, uint32_t* class_len, uint32_t* coverage,
                              uint32_t* mismatches);
/* map_read_to_nodes (src/pseudoaligner.rs:54-61, test surface): node ids in visit order. */
int pa_map_read_to_nodes(pa_index* idx, const uint8_t* ascii, uint32_t len, uint32_t allowed_mismatches,
                         uint32_t* node_buf, uint32_t node_cap, uint32_t* num_nodes, uint32_t* coverage,
                         uint32_t* mismatches);

/* node lists of a whole batch (test surface): nodes_flat[i*nodes_stride ..] holds the first min(nodes_len[i],
 * nodes_stride) node ids of read i */
int pa_map_batch_nodes(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n_reads,
                       uint32_t allowed_mismatches, pa_read_result* results, uint32_t* nodes_flat, uint32_t nodes_stride,
                       uint32_t* nodes_len);

/* process_reads (src/pseudoaligner.rs:420-514): FASTQ in, one Debug-formatted tuple per read on `out_path`
 * ("-" = stdout) in INPUT order (the reference's order is completion order, :490). num_threads sizes the
 * host parse/format pool. n_reads_out/n_flagged_out may be NULL.
 * Input: plain or gzip'ed (multi-member) FASTQ (a gzip'ed file is inflated into host memory first — one zlib stream, some 0.4 GB/s, and the whole
 * text resident: the reference's CLI takes plain files only, src/bin/pseudoaligner.rs:139; inflate large files upstream — or recompress them once with `bgzip`: a file that is BGZF from first byte to last (pa_bgzf_scan accepts it) is NOT inflated by the host. Its members' compressed bytes go to HBM as they lie in the file, window by window, and are inflated there (pa_bgzf_inflate_device's kernel, on the copy stream ahead of the scan); the host inflates, member by member, only the unfinished record in front of a window, the last piece of the text and the rest of a text that is not in four-line shape. A corrupt member ends the call with PA_ERR_FORMAT, "corrupt gzip stream", naming the member's file offset and the reason; unlike the one-stream path, which finds corruption before the output file is created, the output may then already hold the tuples of the windows before. PA_INGEST_BGZF=0 forces the one-stream path) in the four-line form every sequencer writes — "@id ...", sequence, "+...",
 * qualities; LF or CRLF; trailing blank lines tolerated (a last record with an empty sequence is still that record). A file whose records are not four lines each (sequence or qualities
 * wrapped over several lines, which bio's reader accepts) is first rewritten into that form by a sequential pass (as many
 * quality lines as sequence lines, as bio 1.5 reads them), then scanned in parallel like any other. PA_ERR_FORMAT with
 * the record number for text that is no FASTQ or ends inside a record. Read ids are cut at the first space, as record.id() does.
 * How it runs (round 6): the host does not look at the text. Worker threads copy WINDOWS of the file into pinned memory (out of the file's
 * mapping with streaming stores; 64 MiB each, PA_INGEST_WINDOW overrides), a window goes to HBM as it is on a copy stream, the GPU finds its records (line breaks, '@' / '+'
 * markers, record.id(), record.seq(): csrc/fastq_scan.hip) and the encode / map / render kernels read sequences and ids where they lie;
 * a window ends where the file offset says, the unfinished record is read again as the head of the next window. The last piece of the
 * text and any text that is not in four-line shape go through the host's tolerant scan (and the same kernels).
 * The pinned host and device buffers of the four windows in flight (about 0.15 GB of each per window for 150-base reads) stay parked
 * on `idx` after a successful call, so that the next file starts with warm buffers; concurrent calls on one index each use their own
 * set; pa_index_destroy frees them. */
int pa_process_reads(pa_index* idx, const char* fastq_path, const char* out_path, int num_threads,
                     uint64_t* n_reads_out, uint64_t* n_flagged_out);
/* process_reads on every GPU it is given — the reference's driver uses every worker it is given (src/pseudoaligner.rs:434-474).
 * idx[0 .. n_idx) are replicas of ONE index (pa_index_create_multi: one handle per GPU of the node); the windows of the text are dealt
 * round-robin to the handles, each with its own streams and buffers, and the tuples are written in INPUT order: the output is byte for
 * byte that of pa_process_reads on one handle. A handle may be listed more than once (it then serves several windows at a time on
 * streams of its own: two lanes on one GPU). PA_ERR_INVALID_ARG when the handles are not replicas (k, nodes, classes, k-mers). */
int pa_process_reads_multi(pa_index* const* idx, int n_idx, const char* fastq_path, const char* out_path, int num_threads,
                           uint64_t* n_reads_out, uint64_t* n_flagged_out);

/* process_reads for a caller that HOLDS the reader. The reference's signature consumes an open fastq::Reader
 * (src/pseudoaligner.rs:420-425), so its drop-in replacement cannot ask for a path: the caller pushes the records it reads —
 * ids as record.id() returns them (:456), sequences as record.seq() (:449), both concatenated with offsets[n+1] — and pulls the
 * reference's Debug tuples (:490), one line per record, in PUSH order. Behind the two calls runs the batch pipeline of
 * pa_process_reads: a full batch (batch_reads, 0 = 2 Mi reads) is packed by `num_threads` workers (0 = all usable CPUs) and
 * launched on the stream's own HIP stream while the caller goes on reading; the batch before it is rendered meanwhile.
 *   push   copies the records (the caller's buffers are free afterwards); may pack + launch a batch and render the previous one
 *   pull   copies rendered text into buf, whole lines only, never waits for the GPU; *n_bytes = 0: nothing ready yet. A buffer that
 *          cannot hold even the next tuple gets PA_ERR_BUFFER_TOO_SMALL with *n_bytes = the bytes that tuple needs (nothing is lost:
 *          pull again with a larger buffer; this failure is not sticky)
 *   flush  launches what is left, waits and renders: afterwards pull drains every record pushed so far
 * One thread at a time per stream object; several objects may share an index. A failure is sticky: every later call on the
 * object returns it. */
typedef struct pa_record_stream pa_record_stream;
int pa_record_stream_create(pa_index* idx, int num_threads, uint64_t batch_reads, pa_record_stream** out);
/* The same over several handles of one index (pa_index_create_multi: the GPUs of a node; a handle may be listed twice): full batches go round-robin to the
 * handles, each on its own stream with its own buffers, and the tuples come back in PUSH order — byte for byte what one handle gives. (The reader-fed form is
 * bound by its reader long before one GPU is: INTEGRATION.md §1; this entry is for callers that parse FASTQ on many threads of their own.) */
int pa_record_stream_create_multi(pa_index* const* idx, int n_idx, int num_threads, uint64_t batch_reads, pa_record_stream** out);
int pa_records_push(pa_record_stream* s, const uint8_t* ids, const uint64_t* id_offsets, const uint8_t* seqs,
                    const uint64_t* seq_offsets, uint64_t n_records);
int pa_records_pull(pa_record_stream* s, char* buf, size_t cap, size_t* n_bytes);
int pa_records_flush(pa_record_stream* s);
/* records rendered so far and how many of them carry the flag of :455 (coverage >= 32 and an empty class) */
int pa_record_stream_stats(const pa_record_stream* s, uint64_t* n_reads, uint64_t* n_flagged);
void pa_record_stream_destroy(pa_record_stream* s);

/* Measurement (bench.py's ingest leg): wall seconds the HOST stages of the last pa_process_reads[_multi] call of this thread /
 * of a record stream since its creation took — the stages run one after the other on the caller's thread, each spread over
 * the worker pool, while the GPU works on the windows before: out[0] scan (record boundaries found by the HOST: the end of the text,
 * text that is not in four-line shape; 0 for a record stream), out[1] pack (pa_process_reads: reading the windows' text into pinned
 * memory; a record stream: gathering ids and sequences), out[2] waiting for the GPU (a window's scan, its kernels), out[3] launch,
 * out[4] waiting for the rendered tuples, out[5] waiting for the writer (0 for a record stream), out[6] the whole call (streams: the
 * sum of the others), out[7] reads. The paired drivers (pa_count_cells, pa_write_bus, pa_count_pairs) report through the same getter, with
 * the meanings their own comments give. */
#define PA_INGEST_STAGES 8
/* What the last pa_process_reads[_multi] call of this thread read: out[0] text_kind (0 a plain mapped file, 1 gzip inflated by the host, 2 BGZF inflated on
 * the GPU), out[1] members of the file (0 unless BGZF), out[2] members inflated on the GPU (launches: a member of a window that was read twice counts twice),
 * out[3] members inflated by the host, out[4] bytes copied host to device as input (text, compressed bytes, member rows, record tables), out[5] bytes of text
 * that first existed in HBM. */
#define PA_INGEST_INPUT_STATS 6
int pa_process_reads_input_stats(uint64_t out[PA_INGEST_INPUT_STATS]);
int pa_process_reads_stage_seconds(double out[PA_INGEST_STAGES]);
int pa_record_stream_stage_seconds(const pa_record_stream* s, double out[PA_INGEST_STAGES]);

/* The scan stage of pa_process_reads by itself, without a GPU: the number of records of a FASTQ file (plain, gzip'ed or with
 * wrapped lines: same acceptance rules and errors as above) and, for the first `capacity` of them, where the record starts,
 * how many bytes its header line has before the line feed ('@' included, and the CR of a CRLF file) and how many bases its
 * sequence has. The sequence begins at start + header_len + 1. Offsets refer to the text as scanned: *text_kind = 0 the file itself, 1 the inflated gzip stream, 2 the text
 * rewritten into four-line records (a file that is in four-line shape at first and wrapped further on is rewritten from the first scan
 * window that is not in shape: offsets of the records from there on refer to the rewritten rest). Every output pointer but n_records may be NULL. */
int pa_fastq_scan_host(const char* fastq_path, int num_threads, uint64_t* n_records, uint64_t* starts, uint32_t* header_len,
                       uint32_t* seq_len, uint64_t capacity, int* text_kind);

/* ---------------- BGZF: blocked gzip (bgzip / htslib), inflated on the GPU ----------------
 * A BGZF file is a multi-member gzip whose members hold at most 64 KiB of text each and carry their own size in a "BC" extra subfield,
 * so that the members are found without inflating and are independent of each other. One row of the member table per member: */
typedef struct pa_bgzf_member {
    uint64_t in_off;     /* first byte of the member's DEFLATE payload in the compressed bytes */
    uint64_t out_off;    /* sum of the ISIZE of the members before it */
    uint64_t file_off;   /* where the member (its gzip header) starts in the compressed bytes: for error messages */
    uint32_t in_len;     /* payload bytes */
    uint32_t out_len;    /* ISIZE, 0 .. 65536 */
    uint32_t crc32;      /* CRC-32 of the text, from the trailer */
    uint32_t reserved;   /* 0 */
} pa_bgzf_member;
#define PA_BGZF_MAX_ISIZE 65536u
/* Host only. Walks data[0, size) from gzip header to gzip header, hopping by BSIZE, and returns PA_OK only if the bytes are BGZF from first
 * to last: every member has the magic 1f 8b 08 with FEXTRA set and no reserved flag, a "BC" subfield of length 2 anywhere among its
 * subfields (which fill XLEN exactly), FNAME / FCOMMENT / FHCRC skipped where present, a block that lies inside the bytes and holds
 * header and trailer, and ISIZE <= 65536. Anything else (ordinary gzip, a truncated last member, a BSIZE that points past the end, no bytes
 * at all) is PA_ERR_NOT_BGZF with *n = 0 and *text_bytes = 0. A file without the 28-byte EOF block is accepted, and so are empty members
 * anywhere. *n = the members, *text_bytes = the sum of ISIZE. members == NULL only counts; otherwise the first min(*n, cap) rows are
 * written and PA_ERR_BUFFER_TOO_SMALL is returned when cap < *n. */
int pa_bgzf_scan(const uint8_t* data, uint64_t size, pa_bgzf_member* members, uint64_t cap, uint64_t* n, uint64_t* text_bytes);
/* d_status[i] of pa_bgzf_inflate_device: 0, or why member i is refused. The verdict is zlib's: a member is accepted exactly when zlib
 * inflates its payload as one raw DEFLATE stream that ends inside the payload's last byte, gives out_len bytes and has the trailer's CRC-32. */
#define PA_INFLATE_OK 0u
#define PA_INFLATE_BAD_MEMBER 1u          /* the table row itself: payload beyond comp_bytes, out_len > 65536, text beyond text_cap */
#define PA_INFLATE_BAD_BLOCK_TYPE 2u      /* reserved block type 3 */
#define PA_INFLATE_STORED_LEN 3u          /* stored block: NLEN is not the complement of LEN */
#define PA_INFLATE_TOO_MANY_SYMBOLS 4u    /* dynamic block: more than 286 literal/length or 30 distance codes */
#define PA_INFLATE_BAD_CODE_LENGTHS 5u    /* over-subscribed code, or an incomplete one that is not a single code of one bit */
#define PA_INFLATE_BAD_REPEAT 6u          /* code 16 with nothing to repeat, or a repeat that runs past HLIT + HDIST */
#define PA_INFLATE_NO_END_OF_BLOCK 7u     /* dynamic block without a code for symbol 256 */
#define PA_INFLATE_BAD_SYMBOL 8u          /* unused code, literal/length symbol 286 / 287, distance symbol 30 / 31 */
#define PA_INFLATE_DISTANCE_TOO_FAR 9u    /* a match reaches in front of the member's first byte */
#define PA_INFLATE_INPUT_EXHAUSTED 10u    /* the payload ends inside the stream */
#define PA_INFLATE_TRAILING_INPUT 11u     /* the stream ends before the payload's last byte */
#define PA_INFLATE_OUTPUT_TOO_LONG 12u    /* more text than ISIZE */
#define PA_INFLATE_OUTPUT_TOO_SHORT 13u   /* less */
#define PA_INFLATE_CRC_MISMATCH 14u
/* Inflates the members d_members[0, n_members) (a device copy of rows of the table above, in_off relative to d_comp) on HIP device `device`,
 * asynchronously on `stream`: member i's text goes to d_text[out_off_i - out_off_0 ...), so a run of consecutive rows can be passed as it
 * stands in the table. One wave per member; a member whose status is not 0 may have written any part of ITS out_len bytes, and nothing is
 * ever written outside a member's own bytes or read outside its own payload. d_status[n_members]. PA_ERR_INVALID_ARG for null pointers;
 * corrupt payloads are not an error of the call: they are the statuses. */
int pa_bgzf_inflate_device(int device, const uint8_t* d_comp, uint64_t comp_bytes, const pa_bgzf_member* d_members, uint64_t n_members,
                           uint8_t* d_text, uint64_t text_cap, uint32_t* d_status, void* stream);
/* the name of a status above ("crc mismatch"), for messages; "unknown" beyond them */
const char* pa_inflate_status_name(uint32_t status);

/* ---------------- equivalence-class count table (multi-GPU reduction unit) ---------------- */
/* counts[c] += number of reads whose class equals index class c; reads with a novel (non-index)
 * non-empty class are counted in counts[num_classes] ("novel"), empty-class mapped reads in
 * counts[num_classes+1], unmapped reads in counts[num_classes+2]. d_counts is a caller-owned device
 * array of pa_counts_len(idx) u64 (so that the caller can all-reduce it with RCCL). */
uint64_t pa_counts_len(const pa_index* idx);
int pa_counts_accumulate_device(pa_index* idx, const pa_read_result* d_results, const uint32_t* d_arena,
                                const uint32_t* d_colour, uint64_t n_reads, uint64_t* d_counts, void* stream);

/* Per-barcode (single-cell) counts, SURVEY.md §8f.3 (the reference's stated purpose, README.md:3): d_barcode[i] = index of the
 * cell barcode of read i (assigned by the host from the barcode read / whitelist). Output = the sparse matrix
 * (barcode, column) -> reads as sorted unique keys (barcode << 32 | column) with their counts, columns as in the dense
 * table (class id, pa_counts_len-3.. = novel / empty / unmapped). d_keys / d_vals are caller-owned device arrays of n_reads
 * entries (the worst case); *n_entries (host) receives the number of non-zero cells. barcode_bits: bits of the barcode
 * index that can be set (0 = all 32; fewer bits = fewer sort passes). Synchronous on `stream`. */
int pa_counts_by_barcode_device(pa_index* idx, const pa_read_result* d_results, const uint32_t* d_arena,
                                const uint32_t* d_barcode, uint64_t n_reads, uint32_t barcode_bits, uint64_t* d_keys,
                                uint32_t* d_vals, uint64_t* n_entries, void* stream);

/* ---------------- single-cell UMI count matrix (10x Chromium: R1 = cell barcode + UMI, R2 = cDNA) ----------------
 * R1 bases [0, bc_len) are the barcode, [bc_len, bc_len + umi_len) the UMI (both lengths 1..16); only the bytes A C G T are bases, any other
 * byte is an N. Per read, in this order:
 *   barcode   in the whitelist: exact; else (no N) the one whitelist barcode among its 3 bc_len single substitutions, or (exactly one N)
 *             the one among the 4 bases at the N; none, several or two Ns: invalid. An R1 shorter than bc_len + umi_len: invalid
 *   UMI       an N drops the read; else packed 2 bits per base, first base most significant (integer order = string order)
 *   gene      R2 mapped as map_read maps it (PA_DEFAULT_ALLOWED_MISMATCHES); confidently mapped = mapped, non-empty class whose
 *             transcripts (tx_gene) all belong to one gene; everything else drops
 * Per (cell, gene), with n(u) = reads of UMI u: every UMI moves to the greatest of {u} and its Hamming-1 neighbours present in the
 * group, ordered by (n, UMI value) — one step, not transitive. Per (cell, corrected UMI) across genes the gene with strictly the most
 * reads keeps the molecule (a tie drops it everywhere). Matrix entry (cell, gene) = distinct surviving UMIs.
 * The molecule key packs cell | gene | UMI in 64 bits: bits(n_whitelist - 1) + bits(num_genes - 1) + 2 umi_len > 64 is PA_ERR_UNSUPPORTED.
 * stats[PA_CELL_STATS]: [0] reads, [1] barcode exact, [2] barcode corrected, [3] barcode invalid, [4] UMI invalid, [5] not confidently
 * mapped, [6] reads counted, [7] UMIs corrected (moved), [8] molecules lost to gene conflicts, [9] UMIs in the matrix (after finish);
 * [0] = [3] + [4] + [5] + [6] and [1] + [2] = [4] + [5] + [6]. */
#define PA_CELL_STATS 10
typedef struct pa_cell_counter pa_cell_counter;
/* The counter of one run on idx's GPU. h: the host index idx was created from (its classes give the per-class gene table; class
 * numbering must be idx's), tx_gene[pa_host_index_num_transcripts(h)] < num_genes (pa_host_index_genes gives the reference's),
 * whitelist: n_whitelist * bc_len bytes, no separators, line i = cell i. Every argument is checked before any device call. */
int pa_cell_counter_create(pa_index* idx, const pa_host_index* h, const uint32_t* tx_gene, uint32_t num_genes,
                           const char* whitelist, uint64_t n_whitelist, uint32_t bc_len, uint32_t umi_len, pa_cell_counter** out);
/* One batch: d_results / d_arena as pa_map_batch_device left them for the R2s, d_r1 the R1s (ASCII, back to back, d_r1_offsets[n+1];
 * only the first bc_len + umi_len bytes of each are read). Call any number of times: molecules are collapsed over the whole run.
 * Synchronous on `stream`. PA_ERR_INVALID_ARG after finish. */
int pa_cell_counter_add_device(pa_cell_counter* c, const pa_read_result* d_results, const uint32_t* d_arena,
                               const uint8_t* d_r1, const uint64_t* d_r1_offsets, uint64_t n_reads, void* stream);
/* UMI correction + gene conflicts + count (synchronous); *n_entries = non-zero matrix entries. */
int pa_cell_counter_finish(pa_cell_counter* c, uint64_t* n_entries);
/* the matrix after finish, sorted by (cell, gene): cell / gene / umis [n_entries] (cap < n_entries: PA_ERR_BUFFER_TOO_SMALL) */
int pa_cell_counter_matrix(const pa_cell_counter* c, uint32_t* cell, uint32_t* gene, uint32_t* umis, uint64_t cap);
int pa_cell_counter_stats(const pa_cell_counter* c, uint64_t stats[PA_CELL_STATS]);
void pa_cell_counter_destroy(pa_cell_counter* c);
/* Barcode whitelist file (plain or gzip'ed, LF or CRLF, one barcode per line) -> out[n * bc_len] (no separators). out NULL: only *n.
 * PA_ERR_FORMAT naming the line for a wrong length, a non-ACGT byte or a duplicate; cap (barcodes) < n: PA_ERR_BUFFER_TOO_SMALL. Host only. */
int pa_whitelist_load(const char* path, uint32_t bc_len, char* out, uint64_t cap, uint64_t* n);
/* The whole chain from files: R1 / R2 FASTQ (acceptance rules of pa_process_reads, gzip included; equal record counts and equal
 * record.id() after a trailing "/1" or "/2" is cut, else PA_ERR_FORMAT with the record number), the whitelist file, genes from
 * pa_host_index_genes(h) -> out_dir/matrix.mtx (MatrixMarket coordinate integer general: genes x cells, 1-based "gene cell umis"
 * sorted by cell then gene), out_dir/barcodes.tsv (the whitelist barcodes with at least one UMI, in whitelist order = the columns),
 * out_dir/features.tsv ("name\tname\tGene Expression" for every gene). stats may be NULL. Batches of about 2 M pairs; the next batch
 * is read while the GPU maps and counts the one before. pa_process_reads_stage_seconds then reports this call's stages:
 * [0] scan, [1] gather, [2] waiting for the mapping, [3] launch, [4] counting (add_device + finish), [5] writing, [6] whole, [7] pairs.
 * Which input takes which path (pa_count_cells, pa_write_bus and pa_count_pairs alike). DEVICE path: the host does not look at the text — windows of
 * the files (a BGZF file's compressed members) go to HBM, the GPU inflates, finds the records, compares the ids and gathers R2 and the R1 prefix
 * (pa_pairs_gather_device's kernels); only the end of each file, and text that is not in four-line shape, is scanned by the host. It is taken when BOTH
 * files are BGZF; with PA_PAIRS_DEVICE_PLAIN=1 in the environment also when the files are plain text or BGZF in any mix (plain text is on request only
 * until its rate has been measured against the host path's). HOST path (scan, id compare and gather on the worker pool; gzip and BGZF inflated whole by
 * zlib): everything else — a plain file without that request, an ordinary-gzip file on either side, or PA_PAIRS_HOST_SCAN=1. Results and error messages
 * are the same on both. On the device path the stages mean: [0] the host's scan (the tails), [1] reading windows into pinned memory, [2] waiting for
 * the GPU (a window's scan, a batch's gather, the mapping), [3] launch. pa_pairs_input_path says which path the last call took. */
int pa_count_cells(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path,
                   uint32_t bc_len, uint32_t umi_len, const char* out_dir, int num_threads, uint64_t stats[PA_CELL_STATS]);

/* ---------------- BUS output: sorted (barcode, UMI, equivalence class) records ----------------
 * The interchange format of the kallisto | bustools family (Melsted, Ntranos, Pachter 2019): where the cell counter above gives one
 * answer (cells x genes) and drops a read whose class spans two genes, this keeps the class of every (barcode, UMI). No whitelist,
 * no correction, no gene table. Per read, in this order; the first rule that applies decides:
 *   1 r1_short    R1 has fewer than bc_len + umi_len bytes: dropped
 *   2 barcode_n   a barcode byte is not A, C, G or T (lower case is no base): dropped (kallisto substitutes a base; this drops and counts)
 *   3 umi_n       the same for a UMI byte: dropped
 *   4 unmapped    R2 unmapped, or mapped with class_len == 0 (or a reference to an index class without ids): dropped
 *   5 bad_class   a class reference >= num_classes, an arena range not inside [0, arena_len), an id >= T, or an arena list that is
 *                 not strictly ascending: dropped. Nothing outside the given buffers is ever read
 *   6 recorded    kept as (barcode, UMI, ec); barcode and UMI packed 2 bits per base, A=0 C=1 G=2 T=3, first base most significant
 * stats[PA_BUS_STATS]: [0] reads, [1] r1_short, [2] barcode_n, [3] umi_n, [4] unmapped, [5] bad_class, [6] recorded, [7] records
 * (after finish); [0] = [1] + .. + [6].
 * bc_len >= 1, umi_len >= 1, bc_len + umi_len <= 32 (both in one 64-bit word), else PA_ERR_UNSUPPORTED before any device call.
 * ec numbering, a pure function of (index, set of recorded classes); T transcripts, M index classes with at least two ids:
 *   t < T        the set {t} (an index class of one id, an arena list of one id)
 *   T + j        the j-th index class with at least two ids, in class-id order (also an arena list whose content equals it)
 *   T + M + r    the r-th novel class: a recorded list of at least two ids that equals no index class, in lexicographic order of the
 *                ascending id lists ({1,5} < {1,5,7} < {2,3})
 * More than 2^31 - 1 ecs: PA_ERR_UNSUPPORTED. Records: distinct (barcode, UMI, ec), count = its reads (summed as u32, clamped at
 * 2^32 - 1), ascending by barcode, then UMI, then ec; flags = pad = 0. The records, the ec table and so the three files do not
 * depend on how the reads were split into batches nor on where in an arena a list lay. Two different lists under one 64-bit content
 * hash are PA_ERR_INTERNAL naming the hash (never expected). */
#define PA_BUS_STATS 8
typedef struct pa_bus_record {   /* = the 32-byte record of a BUS v1 file, little-endian */
    uint64_t barcode, umi;
    int32_t ec;
    uint32_t count, flags, pad;
} pa_bus_record;
typedef struct pa_bus pa_bus;
/* The writer of one run on idx's GPU. h: the host index idx was created from (its classes number the ecs, its names go to
 * transcripts.txt); it must outlive the writer. Every argument is checked before any device call. */
int pa_bus_create(pa_index* idx, const pa_host_index* h, uint32_t bc_len, uint32_t umi_len, pa_bus** out);
/* One batch: d_results / d_arena[arena_len] as pa_map_batch_device or pa_pairs_combine_device left them, d_r1 the R1s (ASCII, back to
 * back, d_r1_offsets[n+1]; only the first bc_len + umi_len bytes of each are read). Any number of calls. Synchronous on `stream`.
 * PA_ERR_INVALID_ARG after finish. */
int pa_bus_add_device(pa_bus* b, const pa_read_result* d_results, const uint32_t* d_arena, uint64_t arena_len, const uint8_t* d_r1,
                      const uint64_t* d_r1_offsets, uint64_t n_reads, void* stream);
/* Collapse over the run, number the ecs (synchronous). A second call only reports the same numbers. */
int pa_bus_finish(pa_bus* b, uint64_t* n_records, uint32_t* n_ecs);
/* after finish: the records in file order (cap < n_records: PA_ERR_BUFFER_TOO_SMALL) */
int pa_bus_records(const pa_bus* b, pa_bus_record* out, uint64_t cap);
/* after finish: ec e = ids[offsets[e] .. offsets[e + 1]), ascending; offsets[n_ecs + 1]. ids NULL: only *n_ids (offsets may be NULL
 * then); ids_cap < *n_ids: PA_ERR_BUFFER_TOO_SMALL */
int pa_bus_ecs(const pa_bus* b, uint64_t* offsets, uint32_t* ids, uint64_t ids_cap, uint64_t* n_ids);
int pa_bus_stats(const pa_bus* b, uint64_t stats[PA_BUS_STATS]);
/* after finish: out_dir/output.bus (header "BUS\0", u32 version 1, bclen, umilen, tlen = 0, then the records), out_dir/matrix.ec
 * ("ec\tid,id,..." for every ec 0 .. n_ecs - 1, 0-based transcript ids) and out_dir/transcripts.txt (the index's names, one per line) */
int pa_bus_write(const pa_bus* b, const char* out_dir);
void pa_bus_destroy(pa_bus* b);
/* The whole chain from files, as pa_count_cells reads them (same acceptance rules, batches and stage seconds; [4] = add_device +
 * finish, [5] = writing) -> the three files of pa_bus_write in out_dir. stats may be NULL. */
int pa_write_bus(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, uint32_t bc_len, uint32_t umi_len,
                 const char* out_dir, int num_threads, uint64_t stats[PA_BUS_STATS]);

/* ---------------- BUS barcode correction against a whitelist, then the collapse again ----------------
 * The `bustools correct` + re-sort step between pa_bus_finish and the gene counter, on the records where they lie.
 *   whitelist  n_whitelist barcodes of bc_len bases in BUS packing (2 bits per base, A=0 C=1 G=2 T=3, first base most significant),
 *              1 <= n_whitelist <= 2^31 - 1. A value >= 4^bc_len or a value that comes twice is PA_ERR_INVALID_ARG; the message names the
 *              entry, for a duplicate the smaller index of the two. bc_len / umi_len limits are pa_bus_create's (else PA_ERR_UNSUPPORTED)
 *   barcode    per DISTINCT barcode of the input, the first rule that applies decides (the wording is the cell counter's):
 *                exact      it is in the whitelist: it stays
 *                corrected  exactly one of its 3 bc_len single substitutions is in the whitelist: it becomes that one
 *                none       no such substitution: every record of it is dropped
 *                ambiguous  two or more: every record of it is dropped
 *              A BUS record never holds an N (pa_bus drops such reads), so the cell counter's rule for one N has no counterpart here
 *   output     every surviving record carries its target barcode; records that now share (barcode, UMI, ec) become one whose count is the
 *              64-bit sum clamped at 2^32 - 1 (pa_bus_finish's rule); strictly ascending by (barcode, UMI, ec), flags = pad = 0. The ec
 *              table is untouched: an ec that no longer occurs stays in matrix.ec, as with bustools. UMIs are not touched here: that is pa_bus_umi_correct, below
 *   stats[PA_BUS_CORRECT_STATS]: [0] records in, [1] reads in (the sum of the counts, u64), [2] distinct barcodes in, [3] barcodes exact,
 *              [4] barcodes corrected, [5] barcodes without a neighbour, [6] barcodes ambiguous, [7] records of exact barcodes, [8] records
 *              of corrected barcodes, [9] records dropped, [10] reads dropped, [11] records out, [12] distinct barcodes out;
 *              [2] = [3] + [4] + [5] + [6], [0] = [7] + [8] + [9], [11] <= [7] + [8]
 *   independence  the result is a pure function of (records, whitelist as a set): the order of the whitelist does not matter, and two
 *              runs give the same bytes
 * pa_bus_whitelist_pack (host): n * bc_len bytes without separators, as pa_whitelist_load leaves them -> packed[n]; a byte that is not
 * A, C, G or T is PA_ERR_INVALID_ARG naming the entry; bc_len outside 1..31 PA_ERR_UNSUPPORTED.
 * pa_bus_correct_records: host arrays of any origin; idx names the GPU, as for pa_genes_create. in[n] must be strictly ascending by
 * (barcode, UMI, ec) with every barcode < 4^bc_len and every UMI < 4^umi_len, else PA_ERR_INVALID_ARG naming the first offending record;
 * n = 0 is legal. out NULL: only *n_out and the stats; cap < *n_out: PA_ERR_BUFFER_TOO_SMALL (*n_out is set). More than 2^31 - 1
 * records: PA_ERR_UNSUPPORTED. Every host argument is checked before any device call; without a GPU a valid call returns
 * PA_ERR_NO_DEVICE (before idx is looked at). stats may be NULL.
 * pa_bus_correct: in place on a finished writer (PA_ERR_INVALID_ARG before pa_bus_finish). Afterwards pa_bus_records, pa_bus_write and
 * pa_genes_create_from_bus see the corrected records, and a second pa_bus_finish and pa_bus_stats[7] report their number. A failing call
 * leaves the writer as it was. A second call with the same whitelist changes nothing: every barcode is exact.
 * pa_bus_correct_phase_ms: the GPU milliseconds of this thread's last correction: [0] whitelist table (upload, sort, insert), [1] distinct
 * barcodes + the exact probe + the miss list, [2] the neighbour probes of the missed barcodes, [3] rewrite + sort + collapse + records.
 * pa_write_bus_corrected: pa_write_bus with pa_whitelist_load(whitelist_path) -> pa_bus_whitelist_pack -> pa_bus_correct after
 * pa_bus_finish (stage seconds [4] include it). pa_whitelist_load stops at 16 bases: bc_len > 16 is PA_ERR_UNSUPPORTED for the file-level
 * calls only. Either stats may be NULL; bus_stats[7] is the number of corrected records. */
#define PA_BUS_CORRECT_STATS 13
#define PA_BUS_CORRECT_PHASES 4
int pa_bus_whitelist_pack(const char* whitelist, uint64_t n, uint32_t bc_len, uint64_t* packed);
int pa_bus_correct_records(pa_index* idx, const pa_bus_record* in, uint64_t n, uint32_t bc_len, uint32_t umi_len, const uint64_t* whitelist,
                           uint64_t n_whitelist, pa_bus_record* out, uint64_t cap, uint64_t* n_out, uint64_t stats[PA_BUS_CORRECT_STATS]);
int pa_bus_correct(pa_bus* finished, const uint64_t* whitelist, uint64_t n_whitelist, uint64_t stats[PA_BUS_CORRECT_STATS]);
int pa_bus_correct_phase_ms(float out[PA_BUS_CORRECT_PHASES]);
int pa_write_bus_corrected(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path,
                           uint32_t bc_len, uint32_t umi_len, const char* out_dir, int num_threads, uint64_t bus_stats[PA_BUS_STATS],
                           uint64_t correct_stats[PA_BUS_CORRECT_STATS]);

/* ---------------- cell calling on BUS records: barcode table, rank knee, filter ----------------
 * The `bustools whitelist` step (a library without a whitelist file) and the "filtered matrix" step (a whitelist lists possible barcodes,
 * not cells) on the records where they lie: one table over the records, a ranking, a threshold, a compaction.
 *   input      n BUS records, STRICTLY ascending by (barcode, UMI, ec), as pa_bus_finish and pa_bus_correct leave them. bc_len / umi_len
 *              limits are pa_bus_create's (else PA_ERR_UNSUPPORTED)
 *   table      one row per distinct barcode, in ascending barcode order:
 *                records = the number of the barcode's records
 *                umis    = its distinct (barcode, UMI) runs, i.e. molecules. A molecule counts 1 whatever its records' read counts, as
 *                          in pa_genes_*
 *                reads   = the u64 sum of its records' count, not clamped
 *   rank       the 0-based position of the row in the order (umis descending, barcode ascending)
 *   curve      the distinct umis values v_0 > v_1 > ... > v_{D-1}; R_j = the number of barcodes with umis >= v_j
 *   threshold  an integer t >= 1. A barcode is CALLED iff umis >= t. pa_knee_default_params: mode PA_KNEE_CURVE, lower 10, divisor 10,
 *              expected_cells 3000, min_umis 1. Nobody has tuned these defaults on a real library
 *     PA_KNEE_MIN       t = min_umis
 *     PA_KNEE_EXPECTED  the Cell Ranger 2.2 / STARsolo rule, integers only: r = expected_cells / 100 (integer division), lowered to B - 1
 *                       when it is beyond the last of the B rows; m = umis of the row at rank r = v_j for the smallest j with R_j > r;
 *                       t = (m + 9) / 10. B = 0: t = 1
 *     PA_KNEE_CURVE     (default) only j < L counts, where L = the number of values >= lower.
 *                       L = 0: t = lower. L <= 2: k = L - 1. Otherwise x_j = log10(R_j) and y_j = log10(v_j) as doubles;
 *                       dx = x_{L-1} - x_0; dy = y_{L-1} - y_0; s_j = (y_j - y_0) * dx - (x_j - x_0) * dy (the height of the point above
 *                       the chord, times a positive constant); k = the smallest j with the greatest s_j if that s_j > 0, else L - 1.
 *                       t = max(lower, (v_k + divisor - 1) / divisor). The product and difference are evaluated exactly as written, in
 *                       f64, with floating-point contraction off; log10 is libm's. The knee is the curve's upper shoulder; the divisor
 *                       carries the threshold below the cell population, as Cell Ranger 2 does with its 99th percentile
 *   refusals   PA_ERR_INVALID_ARG for lower = 0, divisor = 0, min_umis = 0, expected_cells = 0 or an unknown mode (whatever the mode in
 *              use); for records that are not strictly ascending or out of range the message is pa_bus_correct_records'. More than
 *              2^31 - 1 records: PA_ERR_UNSUPPORTED. Host arguments are checked before any device call; without a GPU a valid call
 *              returns PA_ERR_NO_DEVICE (before idx is looked at)
 *   independence  rows, called list, threshold and stats are a pure function of (records, params): two runs give the same bytes
 *   stats[PA_KNEE_STATS]: [0] records, [1] reads, [2] molecules, [3] distinct barcodes (B), [4] D, [5] L (0 outside PA_KNEE_CURVE),
 *              [6] threshold, [7] barcodes called, [8] molecules of called barcodes, [9] reads of called barcodes;
 *              [7] <= [3], [8] <= [2], [9] <= [1]
 * pa_bus_knee_records: host arrays of any origin; idx names the GPU. rows[*n_rows] in ascending barcode order; called[*n_called] the
 * called barcodes in BUS packing, ascending: it can be passed to pa_bus_correct as it is. rows / called NULL: only the counts and the
 * stats. A cap that is too small: PA_ERR_BUFFER_TOO_SMALL with both counts (and the stats) set. NULL p: the defaults. n = 0 is legal.
 * pa_bus_knee: the same on a finished writer (PA_ERR_INVALID_ARG before pa_bus_finish); the records are read where they lie and the
 * writer is unchanged.
 * pa_bus_knee_phase_ms: the GPU milliseconds of this thread's last knee: [0] table, [1] rank + curve, [2] threshold (host) + called list
 * + rows.
 * pa_bus_keep_records / pa_bus_keep: a pure filter with no neighbour rescue. A record survives iff its barcode is in barcodes[], which must
 * be strictly ascending with every value < 4^bc_len, else PA_ERR_INVALID_ARG naming the entry; n_barcodes = 0 is legal and keeps nothing.
 * Survivors stay in order: they are sorted and distinct as they lie, so there is no sort and no collapse. out NULL: only *n_out and the
 * stats; cap < *n_out: PA_ERR_BUFFER_TOO_SMALL. pa_bus_keep works in place on a finished writer with pa_bus_correct's guarantees: the new
 * records are built beside the old ones and swapped in at the end, a failing call leaves the writer as it was; afterwards pa_bus_records,
 * pa_bus_write, pa_genes_create_from_bus, a second pa_bus_finish and pa_bus_stats[7] see the kept records; the ec table is untouched.
 *   stats[PA_BUS_KEEP_STATS]: [0] records in, [1] reads in, [2] distinct barcodes in, [3] barcodes kept, [4] records out, [5] reads out,
 *              [6] listed barcodes that no record carries
 * pa_write_barcode_ranks_tsv (host): header "barcode\trecords\tumis\treads\trank\tcalled", then one line per row in the order given; the
 * barcode is decoded as barcodes.tsv decodes it (first base most significant).
 * pa_write_bus_called / pa_count_cells_em_called: pa_write_bus / pa_count_cells_em with cell calling after pa_bus_finish.
 *   whitelist_path NULL   knee -> pa_bus_correct(called): `bustools whitelist` + `correct`. An uncalled barcode with exactly one called
 *                         one-substitution neighbour is joined to it, every other uncalled barcode is dropped
 *   whitelist_path given  pa_bus_correct(whitelist) -> knee -> pa_bus_keep(called). (A second correction would move whitelisted, uncalled
 *                         barcodes into called neighbours; the pure filter does not.) pa_write_bus_corrected's rules for the file
 *   Both also write out_dir/barcode_ranks.tsv: the rows of the knee's input table. No barcode called: PA_ERR_FORMAT "no barcode reaches
 *   the threshold of N molecules", with nothing written. correct_stats are the one correction's that ran; any stats may be NULL. */
#define PA_KNEE_CURVE 0
#define PA_KNEE_EXPECTED 1
#define PA_KNEE_MIN 2
#define PA_KNEE_STATS 10
#define PA_KNEE_PHASES 3
#define PA_BUS_KEEP_STATS 7
typedef struct pa_knee_params { uint32_t mode, lower, divisor, expected_cells, min_umis, reserved[3]; } pa_knee_params;
typedef struct pa_bus_barcode_row { uint64_t barcode, reads; uint32_t records, umis, rank, called; } pa_bus_barcode_row;   /* 32 bytes */
void pa_knee_default_params(pa_knee_params* p);
int pa_bus_knee_records(pa_index* idx, const pa_bus_record* in, uint64_t n, uint32_t bc_len, uint32_t umi_len, const pa_knee_params* p,
                        pa_bus_barcode_row* rows, uint64_t rows_cap, uint64_t* n_rows, uint64_t* called, uint64_t called_cap,
                        uint64_t* n_called, uint64_t stats[PA_KNEE_STATS]);
int pa_bus_knee(const pa_bus* finished, const pa_knee_params* p, pa_bus_barcode_row* rows, uint64_t rows_cap, uint64_t* n_rows,
                uint64_t* called, uint64_t called_cap, uint64_t* n_called, uint64_t stats[PA_KNEE_STATS]);
int pa_bus_knee_phase_ms(float out[PA_KNEE_PHASES]);
int pa_bus_keep_records(pa_index* idx, const pa_bus_record* in, uint64_t n, uint32_t bc_len, uint32_t umi_len, const uint64_t* barcodes,
                        uint64_t n_barcodes, pa_bus_record* out, uint64_t cap, uint64_t* n_out, uint64_t stats[PA_BUS_KEEP_STATS]);
int pa_bus_keep(pa_bus* finished, const uint64_t* barcodes, uint64_t n_barcodes, uint64_t stats[PA_BUS_KEEP_STATS]);
int pa_write_barcode_ranks_tsv(const pa_bus_barcode_row* rows, uint64_t n, uint32_t bc_len, const char* path);
int pa_write_bus_called(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path,
                        uint32_t bc_len, uint32_t umi_len, const pa_knee_params* p, const char* out_dir, int num_threads,
                        uint64_t bus_stats[PA_BUS_STATS], uint64_t correct_stats[PA_BUS_CORRECT_STATS], uint64_t knee_stats[PA_KNEE_STATS]);

/* ---------------- cells x genes from BUS records: multi-gene UMIs shared out by EM ----------------
 * The `bustools count --genecounts --em` step on the records where they lie: where pa_cell_counter drops a read whose class spans two
 * genes, this keeps the molecule and lets a per-cell EM divide it among its genes.
 *   inputs     n BUS records, STRICTLY ascending by (barcode, UMI, ec) as pa_bus_finish leaves them; the ec table as a CSR (ec e =
 *              ids[offsets[e] .. offsets[e + 1]), ascending ids < T); tx_gene[T] < num_genes; bc_len, umi_len
 *   G(e)       the gene set of an ec: the ascending distinct tx_gene[t] over t in e (an ec without ids: the empty set)
 *   molecule   a maximal run of records with equal (barcode, UMI). Its gene set is the intersection of G(e) over its records. An empty
 *              intersection drops the molecule (stats[2]). A molecule counts 1 whatever its records' read counts. There is NO barcode
 *              or UMI correction here: those are pa_bus_correct's and pa_bus_umi_correct's steps, ahead of this one
 *   cell       a distinct barcode with at least one kept molecule; cells are numbered in ascending barcode value
 *   rows       of a cell: the distinct gene sets S of its molecules, each with n_S = its molecules. u_g = n_{{g}} (the singleton
 *              rows); the multi rows are those with |S| >= 2; E = the union of the multi rows; M = sum of n_S over the multi rows
 *   PA_GENES_UNIQUE   entry (cell, g) = u_g; the multi rows are dropped (stats[4] counts their molecules); every value is an exact
 *              integer and no iteration is run
 *   PA_GENES_EM (default)
 *     start          alpha_g = u_g + M / |E| for g in E; alpha_g = u_g otherwise, fixed from then on
 *     one iteration  d_S = sum_{g in S} alpha_g over the multi rows;  alpha'_g = u_g + alpha_g * sum_{multi S with g} n_S / d_S
 *                    (a term with d_S = 0 is 0). A cell without multi rows runs no iteration and has alpha_g = u_g exactly
 *     stop           per cell, pa_quant_run's rule on the genes of E: after iteration i >= min_iters when no g has both
 *                    alpha'_g > alpha_change_limit and |alpha'_g - alpha_g| / alpha'_g > alpha_change; looked at every check_every
 *                    iterations (i a multiple of check_every) and at max_iters. A cell that meets it is frozen at that iterate,
 *                    whatever the other cells still do
 *     truncation     after the run every alpha_g < alpha_limit (of E or not) becomes 0 and leaves the matrix
 *     defaults       pa_quant_default_params' (1e-7, 1e-2, 1e-2, 50, 10 000, 10). Nobody has tuned them for single-cell data
 *   matrix     (cell, gene, f64 value) sorted by (cell, gene), zeros left out
 *   independence   what a cell yields (every iterate, its iteration count, its entries) depends on its own records, the tables and the
 *              params alone, not on the other cells; two runs give the same bits. The order of a cell's multi rows (which fixes the
 *              order of every sum) is that of the 64-bit content hashes of their gene sets
 *   errors     records not strictly ascending, an ec outside [0, n_ecs), tx_gene[t] >= num_genes, an ec id >= num_tx or not ascending,
 *              bc_len / umi_len outside pa_bus_create's limits, params not finite, negative, check_every 0 or an unknown mode:
 *              PA_ERR_INVALID_ARG; for a record the message names the first offending one. More than 2^31 - 1 records:
 *              PA_ERR_UNSUPPORTED. Host arguments are checked before any device call; without a GPU pa_genes_create returns
 *              PA_ERR_NO_DEVICE after those checks (before idx, as pa_quant_create). Two different gene sets of one cell under one
 *              64-bit content hash are PA_ERR_INTERNAL naming the hash (never expected).
 * pa_genes_step: every cell with multi rows, exactly n iterations, no stop rule, no freeze. pa_genes_run: stop rule + truncation from
 * the current alpha, its iterations counted from 1; a second call only reports the same numbers, and pa_genes_step after it is
 * PA_ERR_INVALID_ARG. pa_genes_values: the current alpha of every (cell, gene) that has a row, sorted by (cell, gene), zeros kept;
 * barcode[n_cells] the cells' barcodes; any output may be NULL; cap < n_values: PA_ERR_BUFFER_TOO_SMALL. pa_genes_cell_iters: the
 * iterations every cell has run so far (step and run). pa_genes_matrix: after pa_genes_run, else PA_ERR_INVALID_ARG.
 * stats[PA_GENES_STATS]: [0] records, [1] molecules, [2] molecules dropped, [3] unique-gene molecules, [4] multi-gene molecules, [5] cells,
 * [6] cells with multi rows, [7] multi rows after merging equal sets, [8] ids in multi rows, [9] longest multi row, [10] largest degree
 * (multi rows of one cell that hold one gene), [11] largest cell (|E| + multi rows), [12] most iterations run by a cell, [13] cells
 * not converged, [14] matrix entries, [15] cells that took the HBM variant of the EM kernel ([12] .. [15] after pa_genes_run).
 * pa_genes_write (after run): out_dir/matrix.mtx ("%%MatrixMarket matrix coordinate real general", genes x cells, 1-based "gene cell
 * value" lines in (cell, gene) order, doubles as pa_write_abundance_tsv prints them), barcodes.tsv (the cells' barcodes decoded, first
 * base most significant) and features.tsv (as pa_count_cells writes it; h names the genes and must number num_genes of them). */
#define PA_GENES_EM 0
#define PA_GENES_UNIQUE 1
#define PA_GENES_STATS 16
typedef struct pa_genes pa_genes;
typedef struct pa_genes_params { double alpha_limit, alpha_change_limit, alpha_change;
                                 uint32_t min_iters, max_iters, check_every, mode, reserved; } pa_genes_params;
void pa_genes_default_params(pa_genes_params* p);
/* host arrays of any origin (an output.bus + matrix.ec read back, for instance); idx names the GPU; NULL p = defaults */
int  pa_genes_create(pa_index* idx, const pa_bus_record* records, uint64_t n, const uint64_t* ec_offsets, const uint32_t* ec_ids,
                     uint32_t n_ecs, uint32_t num_tx, const uint32_t* tx_gene, uint32_t num_genes, uint32_t bc_len, uint32_t umi_len,
                     const pa_genes_params* p, pa_genes** out);
/* the records of a finished writer, taken where they lie in HBM, with the writer's ec table; tx_gene[the index's transcripts]. The
 * writer is read only during this call */
int  pa_genes_create_from_bus(const pa_bus* finished, const uint32_t* tx_gene, uint32_t num_genes, const pa_genes_params* p, pa_genes** out);
int  pa_genes_step(pa_genes* g, uint32_t n_iters);
int  pa_genes_run(pa_genes* g, uint32_t* max_iters_run, uint64_t* cells_not_converged);   /* either may be NULL */
int  pa_genes_layout(const pa_genes* g, uint64_t* n_cells, uint64_t* n_values);
int  pa_genes_values(const pa_genes* g, uint64_t* barcode, uint32_t* cell, uint32_t* gene, double* alpha, uint64_t cap);
int  pa_genes_cell_iters(const pa_genes* g, uint32_t* iters);   /* [n_cells] */
int  pa_genes_matrix(const pa_genes* g, uint32_t* cell, uint32_t* gene, double* value, uint64_t cap, uint64_t* n_entries);   /* arrays NULL: only *n_entries */
int  pa_genes_stats(const pa_genes* g, uint64_t stats[PA_GENES_STATS]);
int  pa_genes_write(const pa_genes* g, const pa_host_index* h, const char* out_dir);
void pa_genes_destroy(pa_genes* g);
/* The whole chain from two FASTQ files: pa_write_bus's reader, batches and stage seconds up to pa_bus_finish (no BUS file is written),
 * then pa_genes_create_from_bus with pa_host_index_genes(h), pa_genes_run and pa_genes_write into out_dir. Stage seconds [4] = add_device
 * + finish + the gene stage, [5] = writing. stats may be NULL. */
int  pa_count_cells_em(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, uint32_t bc_len, uint32_t umi_len,
                       const pa_genes_params* p, const char* out_dir, int num_threads, uint64_t stats[PA_GENES_STATS]);
/* ... with the barcodes corrected against a whitelist file between pa_bus_finish and the gene stage (the BUS barcode correction section
 * above; pa_write_bus_corrected's rules for whitelist_path and bc_len). Either stats may be NULL. */
int  pa_count_cells_em_corrected(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path,
                                 uint32_t bc_len, uint32_t umi_len, const pa_genes_params* p, const char* out_dir, int num_threads,
                                 uint64_t genes_stats[PA_GENES_STATS], uint64_t correct_stats[PA_BUS_CORRECT_STATS]);
/* ... with cell calling between pa_bus_finish and the gene stage (the cell calling section above; pa_write_bus_called's rules). */
int  pa_count_cells_em_called(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path,
                              uint32_t bc_len, uint32_t umi_len, const pa_knee_params* kp, const pa_genes_params* p, const char* out_dir,
                              int num_threads, uint64_t genes_stats[PA_GENES_STATS], uint64_t correct_stats[PA_BUS_CORRECT_STATS],
                              uint64_t knee_stats[PA_KNEE_STATS]);

/* ---------------- UMI correction on BUS records, ahead of the gene counter ----------------
 * The `bustools umicorrect` / Cell Ranger / STARsolo 1MM step on the records where they lie: a UMI that is one substitution away from a
 * better-supported UMI of the same barcode and can be the same molecule (their gene sets meet) is taken for a sequencing error of it.
 *   input      as for pa_genes_create: n records STRICTLY ascending by (barcode, UMI, ec), the ec table as a CSR, tx_gene[num_tx] < num_genes,
 *              bc_len / umi_len within pa_bus_create's limits
 *   molecule   a maximal run of records with equal (barcode, UMI). n(m) = the u64 sum of its records' counts, not clamped. S(m) = the
 *              intersection of G(e) over its records (pa_genes_*'s definition, above). A molecule with empty S is INERT: it never moves and is
 *              nobody's target; the gene stage drops it as before
 *   neighbours of m = (b, u): the non-inert molecules (b, v) of the SAME barcode with v different from u in exactly one of the umi_len bases and
 *              S(m) and S(v) sharing a gene
 *   PA_UMI_GREATEST (0, default; the cell counter's wording)  m moves to the greatest of {m} and its neighbours in the order (n, UMI value). One
 *              step, not transitive: every decision is taken on the input state. Every move goes to a strictly greater (n, UMI), so there are
 *              no swaps and no cycles
 *   PA_UMI_DIRECTIONAL (1)  the same, but a neighbour v is eligible only if n(v) >= 2 n(m) - 1 (UMI-tools' directional threshold, evaluated
 *              without overflow). Still one step
 *   output     every record of a moved molecule carries its target's UMI; records that now share (barcode, UMI, ec) become one whose count is
 *              the 64-bit sum clamped at 2^32 - 1; strictly ascending by (barcode, UMI, ec), flags = pad = 0. The ec table is untouched. When
 *              u moves to v and v moves to w, u's records end under v and v's own under w: targets are not followed. A second call may
 *              therefore move molecules again; the step is not idempotent
 *   purity     the result is a pure function of (records, tables, mode): two runs give the same bytes, and a barcode's output records depend
 *              on that barcode's input records alone
 *   stats[PA_BUS_UMI_STATS]: [0] records in, [1] reads in (the u64 sum of the counts), [2] molecules in, [3] distinct barcodes, [4] inert
 *              molecules, [5] non-inert molecules with any UMI at one substitution present in their barcode (inert or not), [6] molecules with
 *              at least one neighbour, [7] molecules moved, [8] molecules moved onto a molecule that itself moved, [9] records rewritten (the
 *              records of moved molecules), [10] reads moved (the sum of n over the moved molecules), [11] records out, [12] molecules out,
 *              [13] molecules of the largest barcode, [14] barcodes that took the HBM variant of the search;
 *              [7] <= [6] <= [5] <= [2] - [4], [11] <= [0], [12] <= [2]
 *   errors     pa_genes_create's checks in pa_genes_create's order, the mode standing where the gene counter checks its params: an unknown mode,
 *              bc_len / umi_len outside pa_bus_create's limits, tx_gene[t] >= num_genes, an ec id >= num_tx or not ascending:
 *              PA_ERR_INVALID_ARG; more than 2^31 - 1 records: PA_ERR_UNSUPPORTED; then the records: not strictly ascending, a barcode >=
 *              4^bc_len or a UMI >= 4^umi_len (pa_bus_correct_records' messages), an ec outside [0, n_ecs): PA_ERR_INVALID_ARG naming the
 *              first offending record. Every host argument is checked before any device call; without a GPU a valid call returns
 *              PA_ERR_NO_DEVICE (before idx is looked at). n = 0 is legal. out NULL: only *n_out and the stats; cap < *n_out:
 *              PA_ERR_BUFFER_TOO_SMALL (*n_out is set). stats may be NULL
 * pa_bus_umi_correct: in place on a finished writer (PA_ERR_INVALID_ARG before pa_bus_finish) with the writer's ec table and pa_bus_correct's
 * guarantees: the new records are built beside the old ones, a failing call (a tx_gene entry >= num_genes, for one) leaves the writer as it
 * was; afterwards pa_bus_records, pa_bus_write, pa_bus_knee, pa_genes_create_from_bus, a second pa_bus_finish and pa_bus_stats[7] see the
 * corrected records. tx_gene[the index's transcripts].
 * pa_bus_umi_correct_phase_ms: the GPU milliseconds of this thread's last UMI correction: [0] molecule table (heads, n, S), [1] neighbour
 * search, [2] rewrite + sort + collapse + records, [3] stats.
 * pa_write_bus_umi / pa_count_cells_em_umi: the one file-level entry per output that takes every record step. The barcode steps run exactly as
 * pa_write_bus / _corrected / _called (pa_count_cells_em / ...) run them for that (whitelist_path, call_cells) pair: whitelist_path may be NULL,
 * call_cells 0 skips cell calling (kp is then ignored; NULL kp = the defaults). Then pa_bus_umi_correct(umi_mode) with pa_host_index_genes(h),
 * always the last of the record steps, then the files or the gene stage. barcode_ranks.tsv therefore shows molecule counts BEFORE UMI
 * correction. An unknown umi_mode is refused before a read is mapped. Stage seconds [4] include the UMI correction. The stats of a step that
 * did not run are left untouched; each may be NULL; bus_stats[7] is the number of records written. */
#define PA_UMI_GREATEST 0
#define PA_UMI_DIRECTIONAL 1
#define PA_BUS_UMI_STATS 15
#define PA_BUS_UMI_PHASES 4   /* [0] molecule table (heads, n, S), [1] neighbour search, [2] rewrite + sort + collapse + records, [3] stats */
int pa_bus_umi_correct_records(pa_index* idx, const pa_bus_record* in, uint64_t n, const uint64_t* ec_offsets, const uint32_t* ec_ids,
                               uint32_t n_ecs, uint32_t num_tx, const uint32_t* tx_gene, uint32_t num_genes, uint32_t bc_len, uint32_t umi_len,
                               uint32_t mode, pa_bus_record* out, uint64_t cap, uint64_t* n_out, uint64_t stats[PA_BUS_UMI_STATS]);
int pa_bus_umi_correct(pa_bus* finished, const uint32_t* tx_gene, uint32_t num_genes, uint32_t mode, uint64_t stats[PA_BUS_UMI_STATS]);
int pa_bus_umi_correct_phase_ms(float out[PA_BUS_UMI_PHASES]);
int pa_write_bus_umi(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path, uint32_t bc_len,
                     uint32_t umi_len, int call_cells, const pa_knee_params* kp, uint32_t umi_mode, const char* out_dir, int num_threads,
                     uint64_t bus_stats[PA_BUS_STATS], uint64_t correct_stats[PA_BUS_CORRECT_STATS], uint64_t knee_stats[PA_KNEE_STATS],
                     uint64_t umi_stats[PA_BUS_UMI_STATS]);
int pa_count_cells_em_umi(pa_index* idx, const pa_host_index* h, const char* r1_path, const char* r2_path, const char* whitelist_path,
                          uint32_t bc_len, uint32_t umi_len, int call_cells, const pa_knee_params* kp, uint32_t umi_mode, const pa_genes_params* p,
                          const char* out_dir, int num_threads, uint64_t genes_stats[PA_GENES_STATS],
                          uint64_t correct_stats[PA_BUS_CORRECT_STATS], uint64_t knee_stats[PA_KNEE_STATS], uint64_t umi_stats[PA_BUS_UMI_STATS]);

/* ---------------- transcript abundances: EM over the class-count table (bulk RNA-seq) ----------------
 * The reference stops at equivalence classes; this is the standard abundance model over them (the EM of kallisto / salmon) on the
 * GPU, in f64. Inputs: the dense table class_counts[pa_counts_len] and, optionally, the serialised overflow words (format below,
 * pa_overflow_fetch / pa_overflow_merge / pa_overflow_allgather): the reduction unit as it is after the reduce over GPUs.
 *   eff_t    = max(len_t - mean_read_len + 1, 1) as a double; mean_read_len <= 0: eff_t = len_t
 *   rows     = the index classes with n_c > 0 + every overflow record (ids sorted, count = its 64-bit pair). The tail slots empty and
 *              unmapped never take part; the novel slot only through the overflow records: with overflow words their counts must sum
 *              to class_counts[num_classes] (else PA_ERR_INVALID_ARG), without them the novel reads are left out (stats[6])
 *   N        = sum of n_c over the rows; N = 0 is legal: every output is 0 and no iteration is run
 *   start    alpha_t = N / T for the T transcripts of the index; a transcript that occurs in no row has alpha_t = 0 throughout
 *   one iteration   w_t = alpha_t / eff_t;  d_c = sum_{t in c} w_t;  alpha'_t = w_t * sum_{c with t} n_c / d_c  (a term with d_c = 0 is 0)
 *   stop     after iteration i >= min_iters when no transcript has both alpha'_t > alpha_change_limit and
 *            |alpha'_t - alpha_t| / alpha'_t > alpha_change; looked at every check_every iterations and at max_iters; then every
 *            alpha_t < alpha_limit / 10 becomes 0. The defaults are kallisto's: 50, 10 000, 1e-2, 1e-2, 1e-7; check_every 10
 *   outputs  est_counts_t = alpha_t; tpm_t = 1e6 (alpha_t / eff_t) / sum_s (alpha_s / eff_s), the sum in transcript order on the host;
 *            per gene (pa_host_index_genes) the sums of both in transcript order
 * Counts are converted exactly: a count of 2^53 or more is PA_ERR_UNSUPPORTED. Two runs on one input give bit-identical results.
 * Every argument is checked before any device call; a call that fails leaves the object as it was. Without a GPU pa_quant_create
 * returns PA_ERR_NO_DEVICE (checked after h, p and out, before idx: no index handle can exist there). */
typedef struct pa_quant pa_quant;
typedef struct pa_quant_params { double mean_read_len, alpha_limit, alpha_change_limit, alpha_change;
                                 uint32_t min_iters, max_iters, check_every, reserved; } pa_quant_params;
void pa_quant_default_params(pa_quant_params* p);
int  pa_quant_create(pa_index* idx, const pa_host_index* h, const pa_quant_params* p, pa_quant** out);   /* NULL p = defaults; h: the host index idx was made from */
int  pa_quant_set_counts(pa_quant* q, const uint64_t* class_counts, uint64_t counts_len,
                         const uint32_t* overflow_words, uint64_t n_words);                              /* host arrays; resets alpha to the start */
int  pa_quant_step(pa_quant* q, uint32_t n_iters);            /* exactly n iterations, no stop rule, no truncation */
int  pa_quant_run(pa_quant* q, uint32_t* iters, int* converged);  /* stop rule + truncation, from the current alpha */
int  pa_quant_alpha(const pa_quant* q, double* alpha);        /* current alpha[T] */
int  pa_quant_fetch(const pa_quant* q, double* est_counts, double* tpm, double* eff_len);   /* [T] each; any may be NULL */
int  pa_quant_fetch_genes(const pa_quant* q, double* est_counts, double* tpm);              /* [num_genes]; either may be NULL */
#define PA_QUANT_STATS 8   /* rows, ids (nnz), transcripts with a row, longest row, largest degree, reads used N, novel reads left out, iterations run */
int  pa_quant_stats(const pa_quant* q, uint64_t stats[PA_QUANT_STATS]);
int  pa_write_abundance_tsv(const pa_quant* q, const char* path);   /* header + "target_id\tlength\teff_length\test_counts\ttpm", doubles as pa_write_mappability_tsv prints them */
void pa_quant_destroy(pa_quant* q);

/* ---------------- bootstrap replicates: resampled EM runs, batched on the GPU ----------------
 * A replicate resamples the N reads of the last pa_quant_set_counts with replacement and runs the EM above on the resampled counts;
 * the spread of a transcript's estimates over the replicates is its inferential variance (kallisto -b, salmon --numBootstraps).
 *   reads    numbered 0 .. N-1 in candidate order: the index classes ascending, then the overflow records in record order; candidate i
 *            owns reads [cum_i, cum_i + n_i); a candidate without entries or without reads owns none
 *   draw j of replicate b (b: a global u32 replicate number, j < N): block i = j >> 1 of Philox4x32-10 with the counter
 *            (lo32(i), hi32(i), b, 0) and the key (lo32(seed), hi32(seed)) gives o0..o3; an even j takes x = o0 | o1 << 32, an odd j
 *            x = o2 | o3 << 32; the read picked is p = (x * N) >> 64 (the high half of the 128-bit product); n_r^(b) = the number of
 *            draws whose pick lies in candidate r's interval. All integer: any implementation gives the same counts bit for bit.
 *            Philox4x32-10 known answers (Random123), counter / key -> output:
 *              0 0 0 0 / 0 0                                         -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *              ffffffff x4 / ffffffff x2                             -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *              243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   limits   N >= 2^32 is PA_ERR_UNSUPPORTED for the bootstrap; N = 0 is legal: all counts 0, no iteration, every output 0
 *   EM       per replicate the rules above. Rows are the rows of the original table: a row whose resampled count is 0 stays and
 *            contributes exact zeros. Start alpha_t = N / T for the transcripts that occur in a row of the original table, 0 otherwise.
 *            Iteration, stop rule and truncation are those of pa_quant_run, per replicate: a replicate stops at the first checked
 *            iteration at which its own rule holds and is frozen from then on (no longer read-modified, whatever the others still do)
 *   independence   what replicate b yields (counts, every iterate, its iteration count) depends on (table, params, seed, b) alone: not
 *            on first, n or the other replicates of its batch; two runs give the same bits
 * The batch is extra state of the object: made by pa_quant_bootstrap_draw, dropped by pa_quant_set_counts; alpha, pa_quant_step,
 * pa_quant_run, pa_quant_stats and every other output above never see it. n == 0, n > PA_QUANT_BOOT_MAX_BATCH, first + n beyond 2^32,
 * k >= n: PA_ERR_INVALID_ARG; counts, step, run or fetch without a drawn batch: PA_ERR_INVALID_ARG ("no bootstrap batch drawn"). */
#define PA_QUANT_BOOT_MAX_BATCH 64
int  pa_quant_bootstrap_draw(pa_quant* q, uint64_t seed, uint32_t first, uint32_t n);       /* replicates first .. first+n-1: resample, alpha to the start */
int  pa_quant_bootstrap_counts(const pa_quant* q, uint32_t k, uint64_t* class_counts, uint64_t counts_len,
                               uint64_t* overflow_counts, uint64_t n_records);              /* k-th replicate of the batch as a table pa_quant_set_counts accepts: slot num_classes = sum of its overflow counts, the two other tail slots 0; overflow_counts in record order (n_records = the records of the table set), may be NULL when n_records is 0 */
int  pa_quant_bootstrap_step(pa_quant* q, uint32_t n_iters);                                /* every replicate, exactly n iterations, no stop rule, no freeze */
int  pa_quant_bootstrap_run(pa_quant* q, uint32_t* iters, int* converged);                  /* [n] each, either may be NULL */
int  pa_quant_bootstrap_fetch(const pa_quant* q, double* est_counts, double* tpm);          /* [n][T] replicate-major; current alpha; tpm by the rule above per replicate; either may be NULL */

/* ---------------- paired-end reads: orient the mates, intersect their classes ----------------
 * The index is stranded: a read maps only as it lies on the transcript strand. A pair is brought into that orientation, its
 * mates are mapped by two ordinary pa_map_batch_device launches and a stage behind them combines the two results per pair
 * into ordinary pa_read_result records plus arena ids, which everything downstream (pa_counts_accumulate_device,
 * pa_results_compact_device, the overflow table, pa_quant_*, the reduce over GPUs) takes as it takes reads.
 *   orientation   PA_PAIR_FR: mate 1 as given, mate 2 reverse-complemented; PA_PAIR_RF: mate 1 reverse-complemented, mate 2 as
 *                 given; PA_PAIR_FF: both as given; anything else is PA_ERR_INVALID_ARG
 *   reverse complement   of the PACKED read: base j of the output is 3 - code of base len - 1 - j of the input. A byte the encoder
 *                 packed as some code is complemented as that code (an N that became A comes out as T). Bits beyond len in the
 *                 output words are zero, whatever the input held there; lengths are unchanged
 *   pair result   each mate mapped as map_read_with_mismatch(allowed_mismatches) maps it (src/pseudoaligner.rs:361-376):
 *                   both None          unmapped: mismatches bit 31 clear, coverage 0, class_len 0
 *                   exactly one Some   that mate's class, coverage and mismatches, mapped
 *                   both Some          ids = the sorted intersection of the two id lists (intersect, src/pseudoaligner.rs:389);
 *                                      coverage = cov1 + cov2; mismatches = mm1 + mm2; mapped even when the intersection is empty
 *                                      (class_len 0: counted in the table's "empty" slot)
 *   representation   class_off carries PA_CLASS_REF only if the id list equals that index class; otherwise the ids lie ascending
 *                 in the PAIR arena at class_off. Which of the two forms a result that equals an index class takes is not
 *                 specified. A pair result never points into a mate's arena.
 * pa_revcomp_tiles_device: tiles (layout above) -> tiles, NOT in place (d_tiles_out sized like d_tiles_in; the reads beyond n_reads
 * of the last tile come out as zero words); asynchronous on stream; n_reads = 0 is a no-op.
 * pa_pairs_combine_device: d_res1 / d_arena1 and d_res2 / d_arena2 as two finished pa_map_batch_device launches left them for mate 1
 * and mate 2 of n_pairs pairs -> d_results[n_pairs], ids in d_arena[arena_cap] (at most PA_MAX_ARENA_ENTRIES are used). d_counts
 * (may be NULL): u64[pa_counts_len(idx)], every pair counted once by the rule of the class-count table; with an overflow table
 * attached to idx every result that is no index class and not empty is also filed there, so that sum(overflow record counts) ==
 * counts[num_classes] holds for pairs as for reads. d_scratch: pa_pairs_scratch_bytes(n_pairs) bytes, 256-byte aligned; it holds the
 * control block of the launch (nothing is kept on idx) and must stay untouched until pa_pairs_finish. Asynchronous on stream.
 * pa_pairs_finish: synchronises the stream; PA_OK, or PA_ERR_ARENA_FULL with *arena_needed = a capacity that suffices. On a full
 * arena no word beyond arena_cap was written and every record whose ids did not fit is recognisable: mapped, class_len > 0,
 * class_off == PA_MAX_ARENA_ENTRIES; the pairs were all counted, but a lost result may sit in the "novel" slot whatever its content and
 * is not filed in the overflow table, while the novel results that did fit HAVE been filed: re-run into a count table AND an attached overflow
 * table both restored to what they held before the failed launch (or find the need with d_counts = NULL first: it does not depend on d_counts). Either output may be NULL.
 * stats[PA_PAIR_STATS]: [0] pairs, [1] both mates mapped, [2] mate 1 only, [3] mate 2 only, [4] neither, [5] both mapped and the
 * intersection empty, [6] results by reference, [7] results in the arena; [0] = [1] + [2] + [3] + [4] and [6] + [7] = [0] - [4] -
 * (mapped results whose class is empty). */
#define PA_PAIR_FR 0
#define PA_PAIR_RF 1
#define PA_PAIR_FF 2
#define PA_PAIR_STATS 8
int pa_revcomp_tiles_device(const pa_index* idx, const uint64_t* d_tiles_in, const uint32_t* d_lens, uint64_t n_reads, uint32_t words_per_read,
                            uint64_t* d_tiles_out, void* stream);
size_t pa_pairs_scratch_bytes(uint64_t n_pairs);
int pa_pairs_combine_device(pa_index* idx, const pa_read_result* d_res1, const uint32_t* d_arena1, const pa_read_result* d_res2,
                            const uint32_t* d_arena2, uint64_t n_pairs, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap,
                            uint64_t* d_counts, void* d_scratch, size_t scratch_bytes, void* stream);
int pa_pairs_finish(pa_index* idx, void* d_scratch, void* stream, uint64_t stats[PA_PAIR_STATS], uint64_t* arena_used, uint64_t* arena_needed);
/* The paired form of pa_map_batch: mates as ASCII (concatenated, offsets[n_pairs + 1] each), encode, reverse complement by `orient`,
 * two launches, combine, D2H; grows its arenas on PA_ERR_ARENA_FULL. Outputs as pa_map_batch returns them (class ids as a CSR in pair
 * order, library-owned until the next pa_map_pairs call of this thread). Every argument is checked before any device call. A convenience
 * path, not one to measure: the call makes and frees its own stream, launch context and buffers, and the two mates and the combine run one
 * after the other with a host synchronisation between them. */
int pa_map_pairs(pa_index* idx, const uint8_t* ascii1, const uint64_t* offsets1, const uint8_t* ascii2, const uint64_t* offsets2,
                 uint64_t n_pairs, int orient, uint32_t allowed_mismatches, pa_read_result* results, uint64_t* class_offsets,
                 const uint32_t** class_ids);

/* The class-count table of a paired-end run from its two FASTQ files (plain or gzip'ed; the acceptance rules of pa_process_reads; equal
 * record counts and equal record.id() after a trailing "/1" or "/2" is cut, else PA_ERR_FORMAT with the record number, exactly as
 * pa_count_cells): batches of about 2 Mi pairs (PA_INGEST_BATCH overrides), the next batch gathered while the GPU maps the two mates of the
 * one before (on two streams) and combines them. h_counts[pa_counts_len(idx)] is overwritten; an overflow table attached to idx receives the
 * novel results; *n_pairs and stats[PA_PAIR_STATS] (both may be NULL) are the run's. pa_process_reads_stage_seconds then reports this
 * call's stages: [0] scan, [1] gather, [2] waiting for the mappings, [3] launch, [4] combine + count, [6] whole, [7] pairs. */
int pa_count_pairs(pa_index* idx, const char* r1_path, const char* r2_path, int orient, uint32_t allowed_mismatches, int num_threads,
                   uint64_t* h_counts, uint64_t* n_pairs, uint64_t stats[PA_PAIR_STATS]);

/* ---------------- unstranded libraries: both strands mapped, the two answers merged ----------------
 * In an unstranded library every fragment is read from either strand at random, while the index is stranded. An ITEM (a single read, or
 * a pair) therefore gets two candidate results in the format of pa_read_result plus arena ids, and a stage behind them merges the two
 * per item into ordinary records plus arena ids, which everything downstream takes as it takes reads.
 *   candidates    S (sense):      a read as given;                 a pair by the pair rule on (mate 1, revcomp mate 2) = PA_PAIR_FR
 *                 R (antisense):  the read's reverse complement;   a pair by the pair rule on (revcomp mate 1, mate 2) = PA_PAIR_RF
 *   item result   neither mapped      unmapped: mismatches bit 31 clear, coverage 0, class_len 0, class_off 0
 *                 exactly one mapped  that candidate's ids, coverage and mismatches
 *                 both mapped         the keys (class non-empty, coverage, -mismatches) are compared lexicographically; the larger key
 *                                     wins and the result is that candidate. Equal keys are a TIE: ids = the sorted union of the two
 *                                     lists without duplicates, coverage and mismatches the common values, mapped even when the union
 *                                     is empty
 *                 (two equally good explanations of a fragment that is as likely from either strand are both compatible: the union;
 *                 a weaker hit on the other strand must not dilute a strong one; an empty intersection of mates is worse evidence than
 *                 any non-empty one)
 *   representation   class_off carries PA_CLASS_REF only if the id list equals that index class; otherwise the ids lie ascending in the
 *                 OUTPUT arena at class_off. Which of the two forms a result that equals an index class takes is not specified. A
 *                 result never points into a candidate's arena. Records with class_len == 0 have class_off == 0.
 * pa_strands_merge_device / pa_strands_finish: the contract of pa_pairs_combine_device / pa_pairs_finish with S in the place of mate 1
 * and R in the place of mate 2 — asynchronous on stream; d_scratch of pa_strands_scratch_bytes(n) bytes (0: n is beyond one launch, the
 * pair stage's limit), 256-byte aligned, holding the launch's control block until the finish; d_counts may be NULL, otherwise every item
 * is counted once by the rule of the class-count table and, with an overflow table attached to idx, every result that is no index class
 * and not empty is filed there; n = 0 is valid; PA_ERR_ARENA_FULL comes with an exact *arena_needed (it does not depend on d_counts or
 * on the order the items were handled in), no word beyond arena_cap was written and every lost record is mapped with class_len > 0 and
 * class_off == PA_MAX_ARENA_ENTRIES; what pa_pairs_finish says about re-running a counted launch holds here too.
 * stats[PA_STRAND_STATS]: [0] items, [1] both candidates mapped, [2] S only, [3] R only, [4] neither, [5] ties, [6] results by
 * reference, [7] results in the arena; [0] = [1] + [2] + [3] + [4] and [6] + [7] = [0] - [4] - (mapped results whose class is empty).
 * A STRANDED library shows in them as [2] >> [3] (or the reverse, for the opposite protocol): the cheap check of the library type. */
#define PA_STRAND_FWD 0
#define PA_STRAND_REV 1
#define PA_STRAND_BOTH 2
#define PA_STRAND_STATS 8
size_t pa_strands_scratch_bytes(uint64_t n);
int pa_strands_merge_device(pa_index* idx, const pa_read_result* d_resS, const uint32_t* d_arenaS, const pa_read_result* d_resR,
                            const uint32_t* d_arenaR, uint64_t n, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap,
                            uint64_t* d_counts, void* d_scratch, size_t scratch_bytes, void* stream);
int pa_strands_finish(pa_index* idx, void* d_scratch, void* stream, uint64_t stats[PA_STRAND_STATS], uint64_t* arena_used, uint64_t* arena_needed);
/* pa_map_batch with a strand: PA_STRAND_FWD maps the reads as given (what pa_map_batch returns), PA_STRAND_REV their reverse complements,
 * PA_STRAND_BOTH both and merges the two by the rule above; anything else is PA_ERR_INVALID_ARG. pa_map_pairs_unstranded: pa_map_pairs
 * for an unstranded library — four mappings, the two candidates by two uncounted combines, the merge. Arguments, checks (all before any
 * device call) and output ownership as pa_map_pairs (the class ids are library-owned until this thread's next call of pa_map_pairs or
 * of one of these two). Convenience paths, not ones to measure: each call makes and frees its own stream, launch context and buffers
 * and runs its mappings one after the other with host synchronisations between them. */
int pa_map_batch_strand(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n_reads, int strand, uint32_t allowed_mismatches,
                        pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids);
int pa_map_pairs_unstranded(pa_index* idx, const uint8_t* ascii1, const uint64_t* offsets1, const uint8_t* ascii2, const uint64_t* offsets2,
                            uint64_t n_pairs, uint32_t allowed_mismatches, pa_read_result* results, uint64_t* class_offsets,
                            const uint32_t** class_ids);
/* pa_count_pairs for an unstranded library: the same files, paths (host scan / device path, chosen by the same conditions), batches, error
 * messages and stage-second slots ([2] waiting for the four mappings, [4] the two combines + the merge + count). Per batch both mates and
 * their reverse complements are mapped (four streams), the two candidates combined uncounted, and ONE counted merge goes into the table
 * and an attached overflow table. stats[PA_STRAND_STATS] (may be NULL) are the run's. */
int pa_count_pairs_unstranded(pa_index* idx, const char* r1_path, const char* r2_path, uint32_t allowed_mismatches, int num_threads,
                              uint64_t* h_counts, uint64_t* n_pairs, uint64_t stats[PA_STRAND_STATS]);

/* ---------------- the pair scan on the device: ids compared, R2 and the R1 prefix gathered ---------------- */
#define PA_PAIRS_CTL_WORDS 8            /* u64 words of the control block d_ctl */
#define PA_PAIRS_WHOLE_READ 0xFFFFFFFFu /* prefix: all of R1 */
/* What the paired drivers do per batch on the host today (record.id() of record i of both files compared after a trailing "/1" or "/2"
 * is cut, every R2 sequence and the first `prefix` bytes of every R1 sequence copied back to back), for texts and record tables that lie in
 * HBM. One call handles a SEGMENT: m pairs, record i of d_rec1 with record i of d_rec2, that land at positions [base, base + m) of a batch.
 *   d_text1 / d_text2   the two texts (text1_bytes / text2_bytes of them are readable), any alignment
 *   d_rec1 / d_rec2     m rows of four u32 each, 16-byte aligned: {id offset, id length, sequence offset, sequence length}, offsets into
 *                       the row's own text (the layout the GPU's FASTQ scan writes). A row that points outside its text is not read: the
 *                       pair gets two empty pieces and its batch position is folded into d_ctl[5]
 *   prefix              bytes of every R1 sequence that are kept; PA_PAIRS_WHOLE_READ: all of it
 *   d_bytes1 / d_off1   R1's pieces back to back and their offsets (u64[base + m + 1] at least; d_off1[base + m] = the bytes so far), so that
 *   d_bytes2 / d_off2   piece i of the batch is d_bytes[d_off[i] .. d_off[i + 1]); the same for R2's whole sequences. A piece that
 *                       would end beyond cap1 / cap2 is not written (no byte beyond the capacity ever is); d_ctl[3] / d_ctl[4] still count
 *                       it, so bytes > capacity says that the batch did not fit
 *   d_ctl               u64[PA_PAIRS_CTL_WORDS], on the device: [0] the smallest batch position whose two ids differ (~0: none), [1] the longest
 *                       R1 piece, [2] the longest R2 piece, [3] R1 bytes, [4] R2 bytes, [5] the smallest batch position with a row outside its
 *                       text (~0: none). A call with base == 0 opens a batch and resets the block; later segments of the batch continue it (the
 *                       running byte counts are the bases of their offsets), in call order on one stream
 *   d_scratch           pa_pairs_gather_scratch_bytes(m) bytes (0: m is beyond the 2^30 pairs of one segment), 256-byte aligned, free again
 *                       when the call's work on the stream is done
 * Asynchronous on stream; m = 0 is valid (an empty segment still opens the batch at base == 0 and writes d_off[base]). */
size_t pa_pairs_gather_scratch_bytes(uint64_t m);
int pa_pairs_gather_device(int device, const uint8_t* d_text1, uint64_t text1_bytes, const uint32_t* d_rec1, const uint8_t* d_text2,
                           uint64_t text2_bytes, const uint32_t* d_rec2, uint64_t m, uint32_t prefix, uint64_t base, uint8_t* d_bytes1,
                           uint64_t cap1, uint64_t* d_off1, uint8_t* d_bytes2, uint64_t cap2, uint64_t* d_off2, uint64_t* d_ctl, void* d_scratch,
                           size_t scratch_bytes, void* stream);
/* What this thread's last pa_count_cells / pa_write_bus / pa_count_pairs / pa_count_pairs_unstranded call read: R1's six entries, then R2's, in pa_process_reads_input_stats' meaning
 * (on the host path only text_kind is filled in). pa_pairs_input_path: 1 when that call took the device path, 0 for the host path. */
int pa_pairs_input_stats(uint64_t out[2 * PA_INGEST_INPUT_STATS]);
int pa_pairs_input_path(void);

/* ---------------- novel classes + the reduction over GPUs ---------------- */
/* The dense table counts every result that is no index class in ONE slot (counts[num_classes]). A pa_overflow keeps WHICH
 * id sets those were, keyed by content, on the GPU: attach one to an index and every pa_map_count_batch_device launch files
 * its novel results there (a small follow-up kernel on the same stream). The reduction unit over GPUs is then
 *   dense table      -> pa_counts_allreduce  (RCCL all-reduce, sum of u64[pa_counts_len])
 *   overflow tables  -> pa_overflow_allgather (RCCL all-gather of the serialised tables, merged by content on every rank)
 * and sum(counts of the merged overflow records) == counts[num_classes] of the reduced dense table.
 * Serialised form (u32 words): [0] = records, [1] = words used (this header included), then per record
 * {len, count low, count high, ids[len]}; merged tables are ordered lexicographically by id list (canonical).
 * max_classes / max_ids size the table (distinct novel classes, sum of their lengths); running out is reported by
 * pa_overflow_fetch / pa_overflow_allgather as PA_ERR_ARENA_FULL, never silently. */
typedef struct pa_overflow pa_overflow;
int pa_overflow_create(int device, uint64_t max_classes, uint64_t max_ids, pa_overflow** out);
void pa_overflow_destroy(pa_overflow* ovf);
int pa_overflow_reset(pa_overflow* ovf, void* stream);
int pa_index_set_overflow(pa_index* idx, pa_overflow* ovf);   /* NULL detaches; the table must outlive its attachment */
/* this GPU's table, serialised and canonical, on the host (library-owned until the next call on ovf) */
int pa_overflow_fetch(pa_overflow* ovf, void* stream, const uint32_t** words, uint64_t* n_words);
/* host-side merge of serialised tables (what every rank does with the gathered buffers); out may be NULL to size */
int pa_overflow_merge(const uint32_t* const* bufs, const uint64_t* n_words, int nbufs, uint32_t* out, uint64_t out_cap,
                      uint64_t* out_words);

/* RCCL communicator, one rank per GPU (xGMI). The 128-byte id comes from ONE rank (pa_comm_unique_id) and reaches the
 * others through whatever the host already has (MPI, a file, torch.distributed ...). RCCL is bound at run time: without
 * librccl these calls fail with PA_ERR_UNSUPPORTED, everything else works. comm == NULL means "one GPU": the reduce is a
 * no-op and the gather is pa_overflow_fetch. */
typedef struct pa_comm pa_comm;
int pa_comm_unique_id(uint8_t id[128]);
int pa_comm_create(int device, int nranks, int rank, const uint8_t id[128], pa_comm** out);
void pa_comm_destroy(pa_comm* comm);
int pa_comm_rank(const pa_comm* comm);
int pa_comm_size(const pa_comm* comm);
int pa_counts_allreduce(pa_index* idx, uint64_t* d_counts, pa_comm* comm, void* stream);   /* in place, asynchronous on stream */
int pa_overflow_allgather(pa_overflow* ovf, pa_comm* comm, void* stream, const uint32_t** words, uint64_t* n_words);

/* ---------------- synthetic workloads (BASELINE.json configs; deterministic, counter-based) ------------- */
/* GENCODE-like transcriptome: returns a host index-less transcript set. */
typedef struct pa_txome pa_txome;
int pa_txome_synthesize(uint32_t num_genes, uint32_t target_transcripts, uint64_t seed, pa_txome** out);
/* The same transcriptome (same genes, exons and isoforms for the same seed) with REAL-GRAPH structure added (bench.py's workload
 * "config3r"): interspersed repeats — `families` + `young_families` consensus elements of `element_len` random bases; a gene is hit with
 * probability gene_fraction_ppm / 1e6 and then carries ONE copy of a random family in its last exon ("3' UTR": every isoform that keeps
 * that exon has it), every base of the copy substituted with a probability drawn per copy from [div_lo_ppm, div_hi_ppm] (old families,
 * Alu-like) or [young_div_lo_ppm, young_div_hi_ppm] — and `low_complexity_genes` genes whose last exon ends in a poly-A, (CA)n or (CAG)n
 * tract of 30..89 units. Result: k-mers shared by tens to hundreds of transcripts of unrelated genes (classes far beyond two 32-id
 * windows), branch-dense unitigs inside the elements, self-loops in the tracts. */
typedef struct pa_synth_repeats {
    uint32_t families, element_len, div_lo_ppm, div_hi_ppm;
    uint32_t young_families, young_div_lo_ppm, young_div_hi_ppm;
    uint32_t gene_fraction_ppm, low_complexity_genes;
} pa_synth_repeats;
int pa_txome_synthesize_repeats(uint32_t num_genes, uint32_t target_transcripts, uint64_t seed, const pa_synth_repeats* repeats, pa_txome** out);
int pa_txome_from_host_index(const pa_host_index* h, pa_txome** out);
int pa_txome_from_fasta(const char* fasta_path, pa_txome** out);
int pa_txome_view(const pa_txome* t, const uint64_t** packed, const uint64_t** tx_start, uint32_t* num_tx);
void pa_txome_destroy(pa_txome* t);
/* reads: read i = transcript drawn with probability proportional to (len - read_len + 1), uniform start,
 * forward strand, per-base substitution with probability sub_rate_ppm/1e6; function of (seed, first_read+i) only. */
int pa_simulate_reads_host(const pa_txome* t, uint32_t read_len, uint64_t seed, uint32_t sub_rate_ppm,
                           uint64_t first_read, uint64_t n_reads, uint32_t words_per_read, uint64_t* tiles,
                           uint32_t* lens);
typedef struct pa_txome_device pa_txome_device;
int pa_txome_upload(const pa_txome* t, uint32_t read_len, int device, pa_txome_device** out);
void pa_txome_device_destroy(pa_txome_device* t);
int pa_simulate_reads_device(const pa_txome_device* t, uint64_t seed, uint32_t sub_rate_ppm, uint64_t first_read,
                             uint64_t n_reads, uint32_t words_per_read, uint64_t* d_tiles, uint32_t* d_lens,
                             void* stream);

/* ---------------- misc ---------------- */
uint32_t pa_abi_version(void);
int pa_device_count(void);
const char* pa_last_error(void);
/* HIP-event timing on the stream kernels are launched on (bench.py's roofline leg). */
int pa_event_create(void** ev);
int pa_event_record(void* ev, void* stream);
int pa_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises `stop` */
int pa_event_destroy(void* ev);
/* raw device memory for hosts without their own allocator */
int pa_device_malloc(int device, size_t bytes, void** out);
int pa_device_free(void* p);
int pa_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int pa_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int pa_memset_device(void* dst, int value, size_t bytes, void* stream);
int pa_stream_synchronize(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSEUDOALIGNER_AMD_H */
