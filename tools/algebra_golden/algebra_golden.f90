!==========================================================================!
! algebra_golden: the reference's sparse_matrix_sum / sparse_matrix_product!
! / PtAP / RARt on one case, for the fixtures under tests/golden/algebra.  !
! Only `use`s the reference's modules; compiled against the objects and    !
! .mod files of oracle/build_ref.sh (see make_fixtures.py).                !
!                                                                          !
!   algebra_golden in.bin out.bin                                          !
! in.bin (stream, native endian): int32 op (0 sum, 1 product, 2 PtAP,      !
!   3 RARt), then the two operands X, Y, each: int32 nrow, ncol, ne,       !
!   ei(ne), ej(ne) (1-based), real64 ev(ne).  Each operand is assembled    !
!   the reference's way: ll_graph%add_edge in order, convert to compressed !
!   sparse, csr_matrix%set_graph, zero, set_value in order.                !
! out.bin: X, Y and the result, each as stored (cursor order):             !
!   int32 nrow, ncol, nnz, rows(nnz), cols(nnz), real64 vals(nnz).         !
!==========================================================================!
program algebra_golden
use types, only: dp
use graphs
use sparse_matrices
implicit none
    character(len=512) :: fin, fout
    integer :: u, op
    type(csr_matrix), target :: X, Y, Z

    call get_command_argument(1, fin)
    call get_command_argument(2, fout)
    open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
    read(u) op
    call read_matrix(u, X)
    call read_matrix(u, Y)
    close(u)

    select case (op)
    case (0)
        call sparse_matrix_sum(Z, X, Y)
    case (1)
        call sparse_matrix_product(Z, X, Y)
    case (2)
        call PtAP(Z, X, Y)
    case default
        call RARt(Z, X, Y)
    end select

    open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
    call write_matrix(u, X)
    call write_matrix(u, Y)
    call write_matrix(u, Z)
    close(u)

contains

subroutine read_matrix(u, A)
    integer, intent(in) :: u
    type(csr_matrix), intent(inout) :: A
    integer :: nrow, ncol, ne, k
    integer, allocatable :: ei(:), ej(:)
    real(dp), allocatable :: ev(:)
    class(graph_interface), pointer :: g

    read(u) nrow, ncol, ne
    allocate(ei(ne), ej(ne), ev(ne))
    if (ne > 0) read(u) ei, ej, ev
    allocate(ll_graph :: g)
    call g%init(nrow, ncol)
    do k = 1, ne
        call g%add_edge(ei(k), ej(k))
    enddo
    call convert_graph_type(g, "compressed sparse")
    call A%init(nrow, ncol)
    call A%set_graph(g)
    call A%zero()
    do k = 1, ne
        call A%set_value(ei(k), ej(k), ev(k))
    enddo
end subroutine

subroutine write_matrix(u, A)
    integer, intent(in) :: u
    type(csr_matrix), intent(inout) :: A
    integer, parameter :: batch = 64
    type(graph_edge_cursor) :: cursor
    integer :: edges(2, batch), num, nnz, m
    real(dp) :: vals(batch)
    integer, allocatable :: ri(:), ci(:)
    real(dp), allocatable :: rv(:)

    nnz = A%get_nnz()
    allocate(ri(nnz), ci(nnz), rv(nnz))
    m = 0
    cursor = A%make_cursor()
    do while (.not. cursor%done())
        call A%get_entries(edges, vals, cursor, batch, num)
        ri(m + 1:m + num) = edges(1, 1:num)
        ci(m + 1:m + num) = edges(2, 1:num)
        rv(m + 1:m + num) = vals(1:num)
        m = m + num
    enddo
    write(u) A%nrow, A%ncol, m
    if (m > 0) write(u) ri(1:m), ci(1:m), rv(1:m)
end subroutine

end program algebra_golden
