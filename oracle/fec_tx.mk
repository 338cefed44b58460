# oracle/fec_tx.mk -- TEST INFRASTRUCTURE ONLY (see oracle/README.md): the downlink L1 encode's checkers.
#
#   make -C oracle -f fec_tx.mk oracle   the CPU restatement oracle/fec_tx_oracle.c (with the coder and parity
#                                        registers of fec_oracle.c) -> oracle/libfec_tx_oracle.so (travels to the GPU box)
#   make -C oracle -f fec_tx.mk ref      the reference's BitVector + GSM::Time under the re-enacted encoder flows of
#                                        ref_fec_tx_driver.cpp -> oracle/_ref/libref_fec_tx.so (build container only)
#
# Flags as in oracle/Makefile: the reference's own -O3, no fast-math, -ffp-contract=off.

REF      ?= /root/reference
CXX      ?= g++
CC       ?= gcc
HERE     := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
OUT      := $(HERE)_ref

REFFLAGS := -O3 -g -std=gnu++11 -w -fPIC -shared -ffp-contract=off \
            -include unistd.h -include cstring -include cstdio -include cstdlib \
            -I$(REF)/CommonLibs -I$(REF)/GSM

.PHONY: all ref oracle
all: oracle ref

oracle: $(HERE)libfec_tx_oracle.so

$(HERE)libfec_tx_oracle.so: $(HERE)fec_tx_oracle.c $(HERE)fec_tx_oracle.h $(HERE)fec_oracle.c $(HERE)fec_oracle.h
	$(CC) -O3 -g -std=gnu99 -fPIC -shared -ffp-contract=off -Wall -Wextra \
	   -fopenmp $(HERE)fec_tx_oracle.c $(HERE)fec_oracle.c -lm -o $@

ref:
	@if [ -d $(REF)/GSM ]; then \
	  mkdir -p $(OUT) && \
	  $(CXX) $(REFFLAGS) $(HERE)ref_fec_tx_driver.cpp $(REF)/CommonLibs/BitVector.cpp -o $(OUT)/libref_fec_tx.so && \
	  echo "built $(OUT)/libref_fec_tx.so"; \
	else echo "reference not present at $(REF): skipping oracle/_ref/libref_fec_tx.so"; fi
