/* The reference's FASTA reader includes <zlib.h> and uses nothing of it; this empty stand-in keeps the
 * CPU build of the reference (../Makefile, target `ref`) independent of zlib's development files. */
